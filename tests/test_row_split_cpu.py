"""The batches of tests/_row_split.py expose a host loop that forgot a row offset: shown here with each stage's oracle alone, no GPU.

Every batched stage cuts a call of more rows than one launch carries into several launches and re-bases, per launch, the input rows, the
lengths, the per-row scalars, the outputs and the workspace slices.  For every stage and every ``b < k`` this file computes what the second
launch would give for row ``P + b`` had it dropped one of the first three offsets, and asserts that it is not what the oracle expects:

* input offset dropped: row ``b``'s samples at row ``P + b``'s length (for two-input stages each input alone as well);
* lengths offset dropped: row ``P + b``'s samples cut or extended to ``lengths[b]``;
* both (the whole row ``b`` again, which is what the twin-row tests before these could not tell from a correct run);
* scalars offset dropped, where the stage takes gains: row ``P + b`` with ``gains[b]``.

"Not what the oracle expects" means: further away than the bar the stage's GPU test allows (its largest possible value where the bar is
derived at run time), or at least one bit where the GPU test compares with ==.  An empty row has no samples for an input or a gain to
change; there the lengths fault alone is visible, and at least two rows behind every split are not empty.

A dropped OUTPUT or WORKSPACE offset is not planted here: the second launch then writes over rows of the first and leaves its own rows (or
its slice of the workspace) as they were, and every GPU test of these batches pre-fills its outputs with NaN / a sentinel and, where the C ABI
takes a workspace, fills that with 0xFF bytes: the untouched rows show, and the rows written over fail against the oracle.  (Of the
workspace, that holds for what is read after the launches that wrote it: StoiMeter's kept lists and energies, which its test reads, and the
limiter's envelope between its two calls.  Scratch that one pass of a host loop writes and reads itself may be shared by the passes, which
run in stream order: no output depends on its offset.  DESIGN.md section 6t.)
"""
import re
from pathlib import Path

import numpy as np
import pytest

import _audio_oracle as audio_oracle
import _dtw_oracle as dtw_oracle
import _limiter_oracle as limiter_oracle
import _loudness_oracle as loudness_oracle
import _mel_oracle as mel_oracle
import _pitch_oracle as pitch_oracle
import _row_split as RS
import _stoi_oracle as stoi_oracle
from viettts_amd import _lib

CSRC = Path(__file__).resolve().parents[1] / "viettts_amd" / "csrc"
SPLITS = {"audio": "AUDIO_ROWS_PER_LAUNCH", "mel": "MEL_ROWS_PER_LAUNCH", "pitch": "PITCH_ROWS_PER_LAUNCH", "stoi": "STOI_ROWS_PER_LAUNCH",
          "loudness": "LOUDNESS_ROWS_PER_LAUNCH", "dtw": "DTW_PAIRS_PER_LAUNCH", "limiter": "LIMITER_ROWS_PER_LAUNCH"}


@pytest.mark.parametrize("stage", list(SPLITS))
def test_the_python_constant_is_the_host_loops(stage):
    text = (CSRC / f"{stage}.hip").read_text()
    found = re.findall(r"^constexpr int (ROWS_PER_LAUNCH|PAIRS_PER_LAUNCH) = (\d+);", text, flags=re.M)
    assert len(found) == 1, found
    name, value = found[0]
    assert SPLITS[stage].endswith(name) and int(value) == getattr(_lib, SPLITS[stage])
    if stage == "dtw":  # its own loop (dtw_common.h: dtw_slice carries two lengths per pair) steps by it
        assert len(re.findall(rf"\+= {name}\)", text)) >= 1
    else:  # the host loop is launch_rows.h's, instantiated with the file's constant, and no hand-written one is left
        assert len(re.findall(rf"for_each_launch(?:_off)?<{name}>\(", text)) >= 1 and len(re.findall(rf"\+= {name}\)", text)) == 0


def _faults(bt, result, far, halves=None):
    """Assert that every planted fault is visible on the rows behind the split.  ``result(content, length, scalar)`` is the stage's oracle,
    ``far(want, other)`` whether ``other`` lies outside what the GPU test accepts for ``want``; ``halves(own, other)`` yields the contents
    with one input of a two-input stage taken from the other row."""
    seen = 0
    for b in range(bt.k):
        own, first = bt.kinds[bt.kind[bt.P + b]], bt.kinds[bt.kind[b]]
        want = result(own.content, own.length, own.scalar)
        assert far(want, result(first.content, first.length, first.scalar)), ("the whole row", b)
        assert far(want, result(own.content, first.length, own.scalar)), ("lengths", b)
        if own.length == 0:
            continue
        seen += 1
        for content in [first.content] + (list(halves(own.content, first.content)) if halves else []):
            assert far(want, result(content, own.length, own.scalar)), ("input", b)
        if own.scalar is not None:
            assert far(want, result(own.content, own.length, first.scalar)), ("scalar", b)
    assert seen >= 2


def _bits_differ(a, b):
    return a.shape != b.shape or not np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_the_builder_lays_the_rows_out_as_promised():
    bt = RS.frames_batch(256, False)
    assert bt.N == 259 and bt.rows.shape == (259, RS.FRAME_STRIDE) and not bt.rows.flags.writeable
    assert bt.lengths[:3] == list(RS.FRAME_FRONT) and bt.lengths[256:] == list(RS.FRAME_BEHIND)
    assert max(bt.lengths) == bt.lengths[257] > max(bt.lengths[:256]) and min(bt.lengths) == bt.lengths[256] == 385
    assert len(set(bt.kind[3:256])) == len(RS.FRAME_FILL) and len(bt.kinds) == 3 + 4 + 3  # the oracle runs ten times, not 259
    calls = []
    RS.per_kind(bt, lambda r: calls.append(r.length))
    assert len(calls) == 10
    for b in range(259):
        assert np.array_equal(bt.rows[b], bt.kinds[bt.kind[b]].content) and bt.lengths[b] == bt.kinds[bt.kind[b]].length
    with pytest.raises(AssertionError):  # the longest row before the split
        RS.split_batch(8, bt.kinds[7:10], bt.kinds[:3], bt.kinds[3:7], min_length=385)


@pytest.mark.parametrize("pcm", [False, True], ids=["f32", "pcm16"])
def test_pitch(pcm):
    T = pitch_oracle.num_frames(RS.FRAME_STRIDE)

    def result(content, length, _):
        r = pitch_oracle.yin_f32(content[None], pitch_oracle.DEFAULT, [length])
        w = np.stack([r.f0[0], r.aperiodicity[0], r.candidate[0]])
        pad = np.broadcast_to(np.array([0, 1, 0], np.float32)[:, None], (3, T - w.shape[1]))
        return np.concatenate([w, pad], axis=1)

    _faults(RS.frames_batch(_lib.PITCH_ROWS_PER_LAUNCH, pcm), result, _bits_differ)


@pytest.mark.parametrize("pcm", [False, True], ids=["f32", "pcm16"])
def test_mel(pcm, golden_dir):
    melfb = np.load(golden_dir / "mel_golden.npz")["melfb"]
    T = mel_oracle.num_frames(RS.FRAME_STRIDE)

    def samples(content):
        return content.astype(np.float32) / np.float32(32768.0) if pcm else content

    def result(content, length, _):
        want = np.full((T, 80), np.log(1e-5))
        w = mel_oracle.log_mel_ragged(samples(content)[None].astype(np.float64), [length], melfb)[0]
        want[: w.shape[0]] = w
        return want

    bt = RS.frames_batch(_lib.MEL_ROWS_PER_LAUNCH, pcm)
    # tests/test_gpu_mel.py's bar for this batch: 4 x the float32 restatement's error plus two ulps at the largest output, both over the batch
    e32 = max(np.abs(mel_oracle.log_mel_ragged(samples(r.content)[None], [r.length], melfb, dtype=np.float32)[0] - result(*r)[: mel_oracle.num_frames(r.length)]).max()
              for r in bt.kinds)
    bar = 4.0 * float(e32) + 2.0 ** -22 * max(float(np.abs(result(*r)).max()) for r in bt.kinds)
    assert 0 < bar < 1e-4
    _faults(bt, result, lambda want, other: np.abs(want - other).max() > bar)


def test_audio():
    rates = (16000, 24000)
    So = audio_oracle.out_samples(704, *audio_oracle.ratio(*rates)[:2])

    def result(content, length, _):
        want, bar = np.zeros(So), 0.0
        if length:
            w = audio_oracle.resample(content[:length], *rates)
            e32 = np.abs(audio_oracle.resample(content[:length], *rates, dtype=np.float32).astype(np.float64) - w).max()
            want[: len(w)], bar = w, 4.0 * float(e32) + 2.0 ** -22 * float(np.abs(w).max())  # tests/test_gpu_audio.py's bar
        return want, bar

    bt = RS.audio_batch(_lib.AUDIO_ROWS_PER_LAUNCH)
    _faults(bt, result, lambda want, other: np.abs(want[0] - other[0]).max() > want[1])
    # at equal rates the stage copies: any other samples or length are other bits
    _faults(bt, lambda content, length, _: np.concatenate([content[:length], np.zeros(704 - length, np.float32)]), _bits_differ)


def test_stoi():
    def result(content, length, _):
        return stoi_oracle.measure(content[:length, 0], content[:length, 1])

    def far(want, other):
        if (want.n_frames, want.n_kept, want.n_segments) != (other.n_frames, other.n_kept, other.n_segments) or not np.array_equal(want.energy, other.energy):
            return True  # compared with ==
        return want.n_segments > 0 and max(abs(want.stoi - other.stoi), abs(want.estoi - other.estoi)) > stoi_oracle.BOUND_CAP

    def far_processed(want, other):  # (the energies are the clean signal's: a wrong processed signal shows in the figures, or in the band magnitudes)
        if want.n_segments:
            return max(abs(want.stoi - other.stoi), abs(want.estoi - other.estoi)) > stoi_oracle.BOUND_CAP
        T = max(0, want.n_kept - 1)
        return T > 0 and np.abs(want.mags[1] - other.mags[1]).max() / want.mags.max() > stoi_oracle.BOUND_CAP

    bt = RS.stoi_batch(_lib.STOI_ROWS_PER_LAUNCH)
    _faults(bt, result, far, lambda own, other: [np.stack([other[:, 0], own[:, 1]], axis=1)])  # (with the clean signal's offset dropped alone)
    for b in range(bt.k):  # ... and the processed signal's
        own, first = bt.kinds[bt.kind[bt.P + b]], bt.kinds[bt.kind[b]]
        if own.length:
            swapped = np.stack([own.content[:, 0], first.content[:, 1]], axis=1)
            assert far_processed(result(own.content, own.length, None), result(swapped, own.length, None)), b


def test_loudness():
    cap = 0.1  # LU: the largest value tests/_loudness_oracle.py's bound() can take

    def result(content, length, _):
        return loudness_oracle.measure(content[:length])

    def far(want, other):
        if (want.n_blocks, want.n_gated) != (other.n_blocks, other.n_gated) or want.sample_peak.view(np.uint32) != other.sample_peak.view(np.uint32):
            return True  # compared with ==
        return loudness_oracle.distance(other, want) > cap

    bt = RS.loudness_batch(_lib.LOUDNESS_ROWS_PER_LAUNCH)
    _faults(bt, result, far)
    # normalize: the gain is the per-row scalar, made on the device from the row's own loudness.  With row b's gain the samples of row
    # P + b are off by more than the GPU test lets the gain be off (twice the bound, in dB)
    refs = RS.per_kind(bt, lambda r: loudness_oracle.measure(r.content[: r.length]))
    gains = [float(loudness_oracle.gain(r)) for r in refs]
    ratio = 10.0 ** (2.0 * cap / 20.0)
    seen = 0
    for b in range(bt.k):
        if bt.lengths[bt.P + b]:
            seen += 1
            assert max(gains[b] / gains[bt.P + b], gains[bt.P + b] / gains[b]) > ratio ** 2, (b, gains[b], gains[bt.P + b])
    assert seen >= 2 and gains[bt.P] == 1.0 and bt.lengths[bt.P - 1] > 0 and bt.lengths[bt.P] > 0  # the packed offset of row P: a full running sum
    assert all(r.gate_room >= 0.05 for r in refs)  # the GPU test's guard


@pytest.mark.parametrize("band", [0, RS.DTW_NARROW_BAND])
def test_dtw(band):
    Ta = 44

    def result(content, length, _):
        la, lb = length // 64, length % 64
        total, path_len, span = dtw_oracle.dtw_f32(content[:la], content[Ta : Ta + lb], band)
        assert np.isfinite(total)
        out = np.full(2 + 2 * Ta, -1, np.int64)
        out[0], out[1], out[2 : 2 + 2 * la] = np.float32(total).view(np.uint32), path_len, np.asarray(span).reshape(-1)
        return out

    def halves(own, other):
        yield np.concatenate([other[:Ta], own[Ta:]])  # a's offset dropped
        yield np.concatenate([own[:Ta], other[Ta:]])  # b's

    bt = RS.dtw_batch(_lib.DTW_PAIRS_PER_LAUNCH)
    _faults(bt, result, lambda want, other: not np.array_equal(want, other), halves)
    a, b, las, lbs = RS.dtw_pairs(bt)
    assert max(las) == las[bt.P + 1] > max(las[: bt.P]) and max(lbs) == lbs[bt.P + 1] > max(lbs[: bt.P])
    assert (las[bt.P], las[bt.P + 2]) == (1, 29) and (lbs[bt.P], lbs[bt.P + 2]) == (37, 1)
    if band:  # the band binds: it changes a total behind the split
        assert any(dtw_oracle.dtw_f32(a[n, : las[n]], b[n, : lbs[n]], band)[0] != dtw_oracle.dtw_f32(a[n, : las[n]], b[n, : lbs[n]])[0] for n in bt.behind())


def test_limiter():
    bound = 4 * 4e-6  # the largest value tests/test_gpu_limiter.py lets its bound take

    def result(content, length, gain):
        return limiter_oracle.limit(content[:length], 16000, gain)

    def far(want, other):
        if want.g != other.g:
            return True  # the gain used is compared with ==
        if len(want.y) != len(other.y):
            return True  # the zeros past the row's end, or the samples they should be
        return max(float(np.abs(want.y - other.y).max()), abs(want.min_gain - other.min_gain) * float(want.c)) > bound

    def far_samples(want, other):  # a wrong gain that the results' gains_used would not show: the samples and the minimum gain alone
        return max(float(np.abs(want.y - other.y).max()), abs(want.min_gain - other.min_gain) * float(want.c)) > bound

    bt = RS.limiter_batch(_lib.LIMITER_ROWS_PER_LAUNCH)
    assert _lib.LIMSTREAM_ROWS_PER_LAUNCH == _lib.LIMITER_ROWS_PER_LAUNCH  # the streamed test runs the same batch
    _faults(bt, result, far)
    for b in range(bt.k):
        own, first = bt.kinds[bt.kind[bt.P + b]], bt.kinds[bt.kind[b]]
        assert far_samples(result(own.content, own.length, own.scalar), result(own.content, own.length, first.scalar)), b
    refs = RS.per_kind(bt, lambda r: result(*r))
    assert all(refs[b].min_gain < 1.0 for b in range(bt.k))  # the first rows are limited, as the test they came from asserts
