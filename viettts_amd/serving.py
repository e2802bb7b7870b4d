"""Many sentences, streamed at once: continuous batching on one GPU (new capability — the reference synthesises one sentence per process).

``viettts_amd.streaming`` makes ONE sentence's first samples leave early.  A frame step of the acoustic decoder costs about the same for 1 row as
for 32, so a server holds its listeners as the rows of a slot pool (``AcousticModel.open_pool``: include/vtts_nat.h): a request enters a free slot
at any tick with its own frame cursor, its chunks leave by its own ``stream_plan``, and the slot is reused when it is done.  One round
(:meth:`SpeechPool.step`) is: admit what is queued, decode ``chunk_frames`` ticks, finish the frame windows that came due (one postnet pass),
vocode the chunks that came due (one ragged generator call), copy them out under the next round.

Which windows and chunks are due is host arithmetic on the rows' cursors: :class:`RoundPlanner`, which runs without a GPU.  Every kernel is the
un-pooled path's and none of its sums depends on a row's slot, start tick or neighbours, so a request's samples equal ``synthesize_stream`` of it
alone with the same chunk settings and seed, bit for bit on the bf16 and bf16x3 generators.
"""
from __future__ import annotations

from collections import deque
from dataclasses import dataclass, field
from typing import Dict, Iterator, List, Optional, Sequence, Tuple

import numpy as np

from .dist import HALO_FRAMES
from .streaming import StreamStep, _check_dtype, stream_plan


@dataclass
class _Row:
    id: int
    T: int  # frames kept
    n_frames: int  # frames the acoustic model would generate
    plan: List[StreamStep]
    slot: int = -1
    start: int = 0  # the tick it was admitted at
    next: int = 0  # first step of the plan not yet issued
    finished: int = 0  # the mel is final below here


@dataclass
class Round:
    windows: List[Tuple[int, int, int]] = field(default_factory=list)  # (slot, f0, f1): one ``MelPool.finish`` call
    chunks: List[Tuple[int, int, StreamStep, bool]] = field(default_factory=list)  # (id, slot, step, last): one ragged generator call, in this order
    retired: List[Tuple[int, int]] = field(default_factory=list)  # (id, slot): rows whose last chunk is in ``chunks``; their slots are free again


class RoundPlanner:
    """The pool's clock and bookkeeping, on the host alone.  Requests queue FIFO and take the lowest free slot; a row's cursor is
    ``clamp(tick - start, 0, n_frames)``; a step of its ``stream_plan`` is due once the cursor has reached its ``decode_upto``.  A round's window
    of a row runs from its finished mark to the last due step's ``mel_upto`` and is never wider than :attr:`max_window` (a step that would make it
    wider waits for the next round)."""

    def __init__(self, slots: int, chunk_frames: int = 32, first_chunk_frames: Optional[int] = None):
        if slots < 1 or chunk_frames < 1 or (first_chunk_frames is not None and first_chunk_frames < 1):
            raise ValueError("slots, chunk_frames and first_chunk_frames must be positive")
        self.slots, self.chunk_frames, self.first_chunk_frames = int(slots), int(chunk_frames), first_chunk_frames
        # one step's own window: a chunk, and for a row's first step the generator's halo on top
        self.max_window = max(self.chunk_frames, int(first_chunk_frames or 0)) + HALO_FRAMES
        self.tick = 0
        self.queue: deque = deque()
        self.rows: List[Optional[_Row]] = [None] * self.slots
        self._ids = 0

    def submit(self, T: int, n_frames: int) -> int:
        """Queue a request of ``T`` kept frames out of ``n_frames``; returns its id."""
        row = _Row(self._ids, int(T), int(n_frames), stream_plan(int(T), int(n_frames), self.chunk_frames, self.first_chunk_frames))
        self._ids += 1
        self.queue.append(row)
        return row.id

    def admissions(self) -> List[Tuple[int, int]]:
        """``(id, slot)`` of the queued requests that enter now, oldest first, each into the lowest free slot, at the current tick."""
        out = []
        for slot in range(self.slots):
            if not self.queue:
                break
            if self.rows[slot] is None:
                row = self.queue.popleft()
                row.slot, row.start = slot, self.tick
                self.rows[slot] = row
                out.append((row.id, slot))
        return out

    def advance(self, nticks: int) -> None:
        self.tick += int(nticks)

    def cursor(self, slot: int) -> int:
        row = self.rows[slot]
        return 0 if row is None else min(max(self.tick - row.start, 0), row.n_frames)

    @property
    def idle(self) -> bool:
        return not self.queue and all(r is None for r in self.rows)

    def due(self, cursors: Optional[Dict[int, int]] = None) -> Round:
        """The round's work for the rows' cursors (default: the clock's own; a test passes its own ``{slot: cursor}``), marked as issued."""
        rnd = Round()
        for slot, row in enumerate(self.rows):
            if row is None:
                continue
            cur = self.cursor(slot) if cursors is None else int(cursors.get(slot, 0))
            f0 = row.finished
            while row.next < len(row.plan):
                step = row.plan[row.next]
                if step.decode_upto > cur or step.mel_upto - f0 > self.max_window:
                    break
                row.next += 1
                row.finished = max(row.finished, step.mel_upto)
                rnd.chunks.append((row.id, slot, step, row.next == len(row.plan)))
            if row.finished > f0:
                rnd.windows.append((slot, f0, row.finished))
            if row.next == len(row.plan):
                rnd.retired.append((row.id, slot))
                self.rows[slot] = None
        return rnd


class SpeechPool:
    """A speech server's inner loop on one GPU: ``submit`` requests at any time, call :meth:`step` (or iterate :meth:`drain`) and hand every
    ``(id, samples, last)`` to its listener.  ``slots`` requests are decoded at once, the rest wait FIFO; a request may have ``Lmax`` tokens and
    ``Fmax`` frames.  Chunks are ``chunk_frames`` kept frames, the first ``first_chunk_frames`` if given (``streaming.stream_plan``); samples are
    int16 (``out_dtype="pcm16"``) or float32 host arrays, ``hop * T`` per request in all.  Work is enqueued on torch's current stream.

    ``limit=True``: every request passes the streamed true-peak limiter (``viettts_amd.limiter.LimiterStream`` with one row per slot: a gain of
    ``gain_db``, then a ceiling of ``ceiling_dbtp``), one push per round for all of the round's rows.  A request's samples are then
    ``synthesize_stream``'s of it alone with the same three arguments; they leave ``LimiterStream.latency`` samples late, a row's chunks of one
    round arrive as one part, and a part may be empty.  The limiter is designed for the models' rate (``FLAGS.sample_rate``).

    ``out_rate`` (other than the models' rate): every request's float32 samples, limited or not, then pass the streamed resampler
    (``viettts_amd.audio.ResamplerStream`` with one row per slot), one push per round likewise: ``synthesize_stream``'s samples of the request
    alone with the same ``out_rate``, ``out_samples(hop * T)`` in all."""

    def __init__(self, duration_model, acoustic_model, generator, slots: int, Lmax: int, Fmax: int, chunk_frames: int = 32,
                 first_chunk_frames: Optional[int] = None, out_dtype: str = "pcm16", limit: bool = False, gain_db: float = 0.0,
                 ceiling_dbtp: float = -1.0, out_rate: Optional[int] = None, denoise: Optional[float] = None):
        if denoise is not None:
            raise ValueError("SpeechPool with denoise: a streamed denoiser needs per-row overlap-add state between chunks, which viettts_amd.denoise "
                             "does not keep; denoise whole sentences with synthesize_sentences(..., denoise=S)")
        _check_dtype(out_dtype)
        self.dm, self.am, self.gen, self.out_dtype = duration_model, acoustic_model, generator, out_dtype
        self.planner = RoundPlanner(slots, chunk_frames, first_chunk_frames)
        self.Lmax, self.Fmax = int(Lmax), int(Fmax)
        self.pool = acoustic_model.open_pool(slots, Lmax, Fmax, self.planner.max_window)
        self._req: Dict[int, tuple] = {}  # id -> (tokens, durations in frames, n_frames, seed) until admitted
        self._empty: List[int] = []  # requests with nothing to say (T < 1): answered by the next step
        self._pending = None  # the previous round's chunks on their way to the host
        self.limiter = self.resampler = None
        from .streaming import _converts

        convert = _converts(out_rate)
        # a row's chunks of one round are one push: at most a window and the generator's halo (RoundPlanner.due)
        max_chunk = generator.hop * (self.planner.max_window + HALO_FRAMES)
        if limit:
            from .limiter import default_limiter
            from .nat.config import FLAGS

            self.limiter = default_limiter(generator.device, FLAGS.sample_rate).open_stream(slots, max_chunk, ceiling_dbtp, "f32" if convert else out_dtype)
            self._gain = float(np.float32(10.0 ** (float(gain_db) / 20.0)))
            max_chunk += self.limiter.latency + 15  # a row's last push also flushes the limiter's delay
        if convert:
            from .audio import resampler
            from .nat.config import FLAGS

            self.resampler = resampler(FLAGS.sample_rate, int(out_rate), generator.device).open_stream(slots, max_chunk, out_dtype)

    def submit(self, tokens: Sequence[int], silence_duration: float = -1.0, dropout_seed: Optional[int] = 0) -> int:
        """Queue one sentence (token ids); the duration model runs now, the frame rules are text2mel's (``frame_plan``).  Returns the request's id."""
        from .nat import text2mel as t2m

        toks = [int(t) for t in tokens]
        if not 1 <= len(toks) <= self.Lmax:
            raise ValueError(f"a request has 1 .. {self.Lmax} tokens (got {len(toks)})")
        frames, nfr, trail = t2m.frame_plan([toks], self.dm([toks]), silence_duration)
        n, T = nfr[0], nfr[0] - trail[0]
        if n > self.Fmax:
            raise ValueError(f"the sentence has {n} frames; the pool was opened for {self.Fmax}")
        if n < 1 or T < 1:
            rid = self.planner._ids
            self.planner._ids += 1
            self._empty.append(rid)
            return rid
        rid = self.planner.submit(T, n)
        self._req[rid] = (toks, frames[0], n, dropout_seed)
        return rid

    def submit_text(self, text: str, lexicon, **kw) -> int:
        from .nat import text2mel as t2m

        return self.submit(t2m.text2tokens(text, lexicon), **kw)

    @property
    def idle(self) -> bool:
        return self.planner.idle and self._pending is None and not self._empty

    def step(self) -> List[Tuple[int, np.ndarray, bool]]:
        """One round.  Returns the chunks of the PREVIOUS round, which have landed on the host under this one."""
        import torch

        from .pipeline import _copy_stream
        from .streaming import _copy_out

        dev = self.gen.device
        cur, s_copy = torch.cuda.current_stream(dev), _copy_stream(dev)
        pl, pool = self.planner, self.pool
        dt = np.int16 if self.out_dtype == "pcm16" else np.float32
        out = [(rid, np.zeros((0,), dt), True) for rid in self._empty]
        self._empty = []
        nxt = None
        if not pl.idle:
            for rid, slot in pl.admissions():
                toks, frames, n, seed = self._req.pop(rid)
                pool.admit(slot, toks, frames, n, dropout_seed=seed)
                if self.limiter is not None:
                    self.limiter.reset(slot, self._gain)
                if self.resampler is not None:
                    self.resampler.reset(slot)
            pool.decode(pl.chunk_frames)
            pl.advance(pl.chunk_frames)
            rnd = pl.due()
            if rnd.windows:
                pool.finish(rnd.windows)
            if rnd.chunks:
                hop = self.gen.hop
                fr = [c[2].chunk.hi - c[2].chunk.lo for c in rnd.chunks]
                Ts = -(-max(fr) // 4) * 4  # the slot length a multiple of 4, as pipeline.synthesize_sentences
                batch = torch.zeros((len(fr), Ts, pool.mel.shape[2]), dtype=torch.float32, device=dev)
                for q, (_, slot, step, _) in enumerate(rnd.chunks):
                    batch[q, : fr[q]] = pool.mel[slot, step.chunk.lo : step.chunk.hi]  # device-side copies (plumbing)
                wav = self.gen.forward_ragged(batch, fr)
                # the kept samples of every chunk back to back, the halos cut as streaming._vocode cuts them
                kept = [wav[q, hop * s.chunk.keep_from : hop * (s.chunk.keep_from + s.chunk.t1 - s.chunk.t0)] for q, (_, _, s, _) in enumerate(rnd.chunks)]
                w = torch.cat(kept)
                parts = [(rid, hop * (s.chunk.t1 - s.chunk.t0), last) for rid, _, s, last in rnd.chunks]
                tails = [t for t in (self.limiter, self.resampler) if t is not None]
                if tails:  # one push each: a row's chunks of this round lie back to back in w and count as one
                    rows, merged = [], []
                    for (rid, count, last), (_, slot, _, _) in zip(parts, rnd.chunks):
                        if rows and rows[-1] == slot:
                            merged[-1] = (rid, merged[-1][1] + count, last)
                        else:
                            rows.append(slot)
                            merged.append((rid, count, last))
                    parts = merged
                    for tail in tails:
                        w, emitted = tail.push(w, counts=[c for _, c, _ in parts], last=[z for _, _, z in parts], rows=rows)
                        parts = [(rid, e, last) for (rid, _, last), e in zip(parts, emitted)]
                elif self.out_dtype == "pcm16":
                    from .audio import to_pcm16

                    w = to_pcm16(w.contiguous())
                host, landed = _copy_out(w, cur, s_copy)
                nxt = (host, landed, parts)
            for _, slot in rnd.retired:
                pool.retire(slot)
        if self._pending is not None:
            host, landed, parts = self._pending
            landed.synchronize()
            hn, at = host.numpy(), 0
            for rid, count, last in parts:
                out.append((rid, hn[at : at + count], last))
                at += count
        self._pending = nxt
        return out

    def drain(self) -> Iterator[Tuple[int, np.ndarray, bool]]:
        """Rounds until every request is done."""
        while not self.idle:
            yield from self.step()

    def close(self) -> None:
        if self.pool is not None:
            self.pool.close()
            self.pool = None
        if self.limiter is not None:
            self.limiter.close()
            self.limiter = None
        if self.resampler is not None:
            self.resampler.close()
            self.resampler = None
