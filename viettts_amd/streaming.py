"""One sentence, streamed: audio chunks leave while the acoustic decoder is still running (new capability — the reference computes the whole
mel, then the whole waveform, vietTTS/synthesizer.py:33-39).

The cut is along time.  The decoder runs up to a frame cursor (``AcousticModel.open_stream``: include/vtts_nat.h, the streaming session), the mel
is made final for a frame window (postnet + residual: 10 frames of the decoder's mel on either side), and a chunk of that window is vocoded with
the generator's 13-frame halo (``viettts_amd.dist.plan_chunks``) and copied to pinned host memory while the decoder carries on:

    chunk k keeps frames [t0, t1)  <-  generator on mel[lo, hi), hi = min(T, t1 + 13)  <-  postnet up to hi  <-  decoder up to min(hi + 10, n_frames)

Every kernel is the un-streamed path's and none of its sums depends on where a window or a chunk lies, so the mel equals
``AcousticModel.__call__``'s bit for bit and the samples equal ``longform.synthesize_chunked`` on that mel with the same chunk plan.

    for pcm in stream_text("xin chào", lexicon, out_dtype="pcm16"):   # int16 arrays, 256 * T samples in all
        sink.write(pcm.tobytes())
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Iterator, List, Optional, Sequence

import numpy as np

from .dist import HALO_FRAMES, Chunk, plan_chunks

POSTNET_HALO = 10  # include/vtts_nat.h: VTTS_NAT_POSTNET_HALO = 5 layers x (5 - 1) / 2 taps per side


@dataclass(frozen=True)
class StreamStep:
    chunk: Chunk  # the frames this step's samples cover (t0, t1) and the frames the generator is fed (lo, hi)
    mel_upto: int  # the mel must be final up to here (= chunk.hi)
    decode_upto: int  # ... for which the decoder must have produced the frames up to here


def stream_plan(T: int, n_frames: int, chunk_frames: int, first_chunk_frames: Optional[int] = None, voc_halo: int = HALO_FRAMES,
                post_halo: int = POSTNET_HALO) -> List[StreamStep]:
    """The steps of one streamed sentence.  ``n_frames``: the frames the acoustic model would generate; ``T <= n_frames``: the frames kept (after
    text2mel's trailing-silence trim, vietTTS/nat/text2mel.py:99-102).  Chunks of ``chunk_frames`` kept frames (``plan_chunks``: a generator halo per
    side, none at the utterance's true edges), the first of ``first_chunk_frames`` if given — a short first chunk is what an interactive caller
    hears first.  The decoder is never asked for frames past ``min(T + post_halo, n_frames)``: what the trim would drop is not decoded."""
    if not 1 <= T <= n_frames:
        raise ValueError(f"need 1 <= T <= n_frames (got {T}, {n_frames})")
    if post_halo < 0 or (first_chunk_frames is not None and first_chunk_frames < 1):
        raise ValueError("post_halo must be >= 0 and first_chunk_frames >= 1")
    if first_chunk_frames is None:
        chunks = plan_chunks(T, chunk_frames, voc_halo)
    else:  # the first chunk of a plan in first_chunk_frames, then a plan of the rest moved behind it: halos are cut at the UTTERANCE's edges only
        head = plan_chunks(T, int(first_chunk_frames), voc_halo)[0]
        a = head.t1
        rest = plan_chunks(T - a, chunk_frames, voc_halo) if a < T else []
        chunks = [head] + [Chunk(c.index + 1, c.t0 + a, c.t1 + a, max(0, c.t0 + a - voc_halo), min(T, c.t1 + a + voc_halo)) for c in rest]
    return [StreamStep(c, c.hi, min(c.hi + post_halo, n_frames)) for c in chunks]


def _copy_out(w, cur, s_copy):
    """Device samples -> pinned host memory on the copy stream, behind an event on the compute stream.  Returns (host tensor, landed event)."""
    import torch

    done = torch.cuda.Event()
    done.record(cur)
    host = torch.empty(w.shape, dtype=w.dtype, pin_memory=True)
    s_copy.wait_event(done)
    with torch.cuda.stream(s_copy):
        host.copy_(w, non_blocking=True)
        landed = torch.cuda.Event()
        landed.record(s_copy)
    w.record_stream(s_copy)
    return host, landed


def _vocode(generator, mel, chunk: Chunk, out_dtype: str):
    """The chunk's kept samples on the device: the generator on ``mel[lo:hi]`` (``[T, num_mels]`` rows), its halo's samples dropped."""
    hop = generator.hop
    wav = generator(mel[chunk.lo : chunk.hi].unsqueeze(0).contiguous())
    w = wav[0, hop * chunk.keep_from : hop * (chunk.keep_from + chunk.t1 - chunk.t0)]
    if out_dtype == "pcm16":
        from .audio import to_pcm16

        w = to_pcm16(w.contiguous())
    return w


def _first(*tensors):
    """Element 0 of each device tensor as a float: one read-back."""
    import torch

    return tuple(float(v) for v in torch.stack([t[0] for t in tensors]).tolist())


class _Limited:
    """The streamed true-peak limiter behind one sentence's vocoder chunks (``viettts_amd.limiter.LimiterStream``, one row): a fixed gain of
    ``gain_db`` and a ceiling of ``ceiling_dbtp`` that holds while the sentence is still being decoded.  The limiter is the models' rate's
    (``FLAGS.sample_rate``: the look-ahead in samples and the oversampling filter), as the un-streamed ``limit`` hooks'."""

    def __init__(self, device, max_chunk: int, gain_db: float, ceiling_dbtp: float, out_dtype: str):
        from .limiter import default_limiter
        from .nat.config import FLAGS

        self.stream = default_limiter(device, FLAGS.sample_rate).open_stream(1, max_chunk, ceiling_dbtp, out_dtype)
        self.stream.reset(0, float(np.float32(10.0 ** (float(gain_db) / 20.0))))

    def push(self, w, last: bool):
        """The float32 chunk ``w`` on the device -> the samples that leave now, in the session's out_dtype."""
        return self.stream.push(w, counts=[int(w.numel())], last=last)[0]

    def summary(self) -> dict:
        r = self.stream.results()
        tp, mg, g = _first(r.true_peak, r.min_gain, r.gains)
        return {"true_peak": tp, "min_gain": mg, "gain": g}

    def close(self) -> None:
        self.stream.close()


class _Resampled:
    """The streamed resampler behind one sentence's chunks (``viettts_amd.audio.ResamplerStream``, one row): the models' rate
    (``FLAGS.sample_rate``) to ``out_rate``, ``Resampler`` on the whole waveform bit for bit, ``latency`` input samples late."""

    def __init__(self, device, max_chunk: int, out_rate: int, out_dtype: str):
        from .audio import resampler
        from .nat.config import FLAGS

        self.resampler = resampler(FLAGS.sample_rate, out_rate, device)
        self.stream = self.resampler.open_stream(1, max_chunk, out_dtype)

    def push(self, w, last: bool):
        """The float32 chunk ``w`` on the device -> the samples that leave now, in the session's out_dtype."""
        return self.stream.push(w, counts=[int(w.numel())], last=last)[0]

    def close(self) -> None:
        self.stream.close()


def _converts(out_rate: Optional[int]) -> bool:
    """Does ``out_rate`` ask for a conversion?  None and the models' own rate do not: those calls are the calls without the argument."""
    if out_rate is None:
        return False
    from .nat.config import FLAGS

    if int(out_rate) < 1:
        raise ValueError(f"out_rate must be positive, got {out_rate!r}")
    return int(out_rate) != FLAGS.sample_rate


def _tail(device, max_chunk: int, out_dtype: str, limit: bool, gain_db: float, ceiling_dbtp: float, out_rate: Optional[int]):
    """The un-streamed pipeline's order behind the vocoder's float32 chunks: (limiter, float32 out) -> (resampler, ``out_dtype``).  Returns
    ``(limiter or None, resampler or None)``; with neither the vocoder's chunk leaves as it did."""
    rs = _converts(out_rate)
    lim = _Limited(device, max_chunk, gain_db, ceiling_dbtp, "f32" if rs else out_dtype) if limit else None
    try:  # a limiter's last push also flushes its delay
        res = _Resampled(device, max_chunk + (lim.stream.latency + 15 if lim else 0), int(out_rate), out_dtype) if rs else None
    except Exception:
        if lim is not None:
            lim.close()
        raise
    return lim, res


def _check_dtype(out_dtype: str) -> None:
    if out_dtype not in ("f32", "pcm16"):
        raise ValueError(f"out_dtype must be 'f32' or 'pcm16', got {out_dtype!r}")


def stream_mel(generator, mel, chunk_frames: int = 32, first_chunk_frames: Optional[int] = None, out_dtype: str = "f32", limit: bool = False,
               gain_db: float = 0.0, ceiling_dbtp: float = -1.0, out_rate: Optional[int] = None) -> Iterator[np.ndarray]:
    """Vocoder-only streaming of a finished mel (``[T, num_mels]`` float32, host array or tensor): the chunks of :func:`stream_plan`, one generator
    call each, every chunk's read-back under the next chunk's compute.  Yields host arrays (float32, or int16 equal to ``wavio.float_to_pcm16``
    of the float chunks); their concatenation has ``hop * T`` samples.  With ``limit=True`` every chunk passes the streamed true-peak limiter
    (a gain of ``gain_db``, then a ceiling of ``ceiling_dbtp``) on the device: the samples are ``TruePeakLimiter.limit``'s of the whole
    waveform bit for bit and leave ``LimiterStream.latency`` samples late, so the first chunk is shorter and the last one longer.  With
    ``out_rate`` (other than the models' rate) every chunk then passes the streamed resampler (``viettts_amd.audio.ResamplerStream``): the
    samples are ``Resampler(models' rate, out_rate)``'s of the whole (limited) float32 waveform bit for bit, ``out_samples(hop * T)`` in all."""
    import torch

    from .pipeline import _copy_stream

    _check_dtype(out_dtype)
    if not isinstance(mel, torch.Tensor):
        mel = torch.from_numpy(np.ascontiguousarray(mel, dtype=np.float32))
    if mel.dim() != 2:
        raise ValueError("mel must be [T, num_mels]")
    mel = mel.to(generator.device)
    T = int(mel.shape[0])
    if T < 1:
        return
    cur, s_copy = torch.cuda.current_stream(generator.device), _copy_stream(generator.device)
    pending = None
    plan = stream_plan(T, T, chunk_frames, first_chunk_frames)
    lim, res = _tail(generator.device, generator.hop * max(s.chunk.t1 - s.chunk.t0 for s in plan), out_dtype, limit, gain_db, ceiling_dbtp, out_rate)
    try:
        for k, step in enumerate(plan):
            w = _vocode(generator, mel, step.chunk, "f32" if lim or res else out_dtype)
            if lim is not None:
                w = lim.push(w.contiguous(), k + 1 == len(plan))
            if res is not None:
                w = res.push(w.contiguous(), k + 1 == len(plan))
            nxt = _copy_out(w, cur, s_copy)
            if pending is not None:
                pending[1].synchronize()
                yield pending[0].numpy()
            pending = nxt
        pending[1].synchronize()
        yield pending[0].numpy()
    finally:
        for t in (lim, res):
            if t is not None:
                t.close()


def synthesize_stream(tokens: Sequence[int], duration_model, acoustic_model, generator, silence_duration: float = -1.0, dropout_seed: Optional[int] = 0,
                      dropout_rng=None, chunk_frames: int = 32, first_chunk_frames: Optional[int] = None, out_dtype: str = "f32",
                      info: Optional[dict] = None, limit: bool = False, gain_db: float = 0.0, ceiling_dbtp: float = -1.0,
                      out_rate: Optional[int] = None) -> Iterator[np.ndarray]:
    """A generator over the waveform of ONE sentence (token ids), chunk by chunk, in order: host arrays, float32 or (``out_dtype="pcm16"``) int16 equal
    to ``wavio.float_to_pcm16`` of the float chunks; ``256 * T`` samples in all, T = the frames text2mel keeps.  The frame rules are text2mel's
    (``frame_plan``: vietTTS/nat/text2mel.py:78-79, :90-102); dropout as ``predict_mel`` (``dropout_rng``: the reference's stream; else
    ``dropout_seed``; both None: none).  ``T < 1`` yields nothing.

    Per step of :func:`stream_plan`: decoder up to ``decode_upto``, postnet up to ``mel_upto``, generator on ``mel[lo:hi]``, the kept samples (packed
    to PCM16 on the device if asked) to pinned memory on a copy stream; the NEXT step's decoder frames are enqueued before the host waits for this
    step's copy.  ``info`` (a dict) receives ``frames`` (T), ``n_frames`` and ``samples`` before the first chunk is yielded, and
    ``frames_decoded_at_first_chunk``.  Work is enqueued on torch's current stream.

    ``limit=True``: the vocoder's float32 chunk stays on the device and passes the streamed true-peak limiter (a gain of ``gain_db``, a ceiling of
    ``ceiling_dbtp``: :func:`stream_mel`) before the copy; ``info["limiter"]`` receives ``true_peak``, ``min_gain`` and ``gain`` with the last chunk.

    ``out_rate`` (other than the models' rate): the float32 chunk, limited or not, passes the streamed resampler before the copy
    (:func:`stream_mel`); ``info["samples"]`` is then ``out_samples(hop * T)``.  ``info["sample_rate"]`` is the rate of what is yielded."""
    import torch

    from .nat import text2mel as t2m
    from .pipeline import _copy_stream

    _check_dtype(out_dtype)
    toks = [int(t) for t in tokens]
    secs = duration_model([toks])
    frames, nfr, trail = t2m.frame_plan([toks], secs, silence_duration)
    n, T = nfr[0], nfr[0] - trail[0]
    samples, rate = generator.hop * max(T, 0), t2m.FLAGS.sample_rate
    if _converts(out_rate):
        from math import gcd

        g = gcd(rate, int(out_rate))
        samples, rate = -(-samples * (int(out_rate) // g) // (rate // g)), int(out_rate)  # include/vtts_audio.h: ceil(S L / M)
    if info is not None:
        info.update(frames=max(T, 0), n_frames=n, samples=samples, sample_rate=rate)
    if n < 1 or T < 1:
        return
    plan = stream_plan(T, n, chunk_frames, first_chunk_frames)
    windows = [b.mel_upto - a for a, b in zip([0] + [s.mel_upto for s in plan[:-1]], plan)]
    kw = {"dropout_rng": dropout_rng} if dropout_rng is not None else {"dropout_seeds": None if dropout_seed is None else [dropout_seed]}
    dev = generator.device
    cur, s_copy = torch.cuda.current_stream(dev), _copy_stream(dev)
    lim, res = _tail(dev, generator.hop * max(s.chunk.t1 - s.chunk.t0 for s in plan), out_dtype, limit, gain_db, ceiling_dbtp, out_rate)
    try:
        with acoustic_model.open_stream([toks], [frames[0]], [n], max(windows), **kw) as st:
            st.decode(plan[0].decode_upto)
            final = 0
            for k, step in enumerate(plan):
                if step.mel_upto > final:
                    st.finish(final, step.mel_upto)
                    final = step.mel_upto
                w = _vocode(generator, st.mel[0], step.chunk, "f32" if lim or res else out_dtype)
                if lim is not None:
                    w = lim.push(w.contiguous(), k + 1 == len(plan))
                if res is not None:
                    w = res.push(w.contiguous(), k + 1 == len(plan))
                host, landed = _copy_out(w, cur, s_copy)
                if info is not None and k == 0:
                    info["frames_decoded_at_first_chunk"] = st.frames_decoded
                if k + 1 < len(plan):
                    st.decode(plan[k + 1].decode_upto)  # under this chunk's vocoder and copy
                landed.synchronize()
                if limit and info is not None and k + 1 == len(plan):
                    info["limiter"] = lim.summary()
                yield host.numpy()
    finally:
        for t in (lim, res):
            if t is not None:
                t.close()


def stream_text(text: str, lexicon_fn=None, silence_duration: float = -1.0, out_rate: Optional[int] = None, **kw) -> Iterator[np.ndarray]:
    """:func:`synthesize_stream` from text, through the models ``viettts_amd.nat.text2mel`` and ``viettts_amd.hifigan.mel2wave`` cache (the
    checkpoints under the CWD, as the reference reads them); the dropout stream is ``predict_mel``'s.  ``out_rate``: as there."""
    from .hifigan.mel2wave import _generator
    from .nat import text2mel as t2m

    tokens = t2m.text2tokens(text, t2m.FLAGS.data_dir / "lexicon.txt" if lexicon_fn is None else lexicon_fn)
    am = t2m.acoustic_model()
    if "dropout_rng" not in kw and getattr(am, "checkpoint_rng", None) is not None:
        kw["dropout_rng"] = am.checkpoint_rng
    return synthesize_stream(tokens, t2m.duration_model(), am, _generator(), silence_duration, out_rate=out_rate, **kw)
