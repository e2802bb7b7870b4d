"""The audio stage's kernel (viettts_amd/csrc/audio.hip, include/vtts_audio.h) on the GPU against the fp64 oracle.

The bar, for every input and over EVERY element of the output:

    |gpu - fp64|  <=  4 * err_ref32 + 2^-22 * max |fp64|

``err_ref32`` is the largest error against fp64 of the oracle's fp32 restatement (tests/_audio_oracle.py: fp32 samples and taps, one
fused multiply-add chain in ascending n) on that input; it is never taken from the kernel under test.  The second term is two fp32
ulps at the largest output.  PCM16 output has conditions of its own (below).
"""
import ctypes as C

import numpy as np
import pytest
import torch

import _audio_oracle as oracle
import _row_split as RS
from viettts_amd import _lib, wavio
from viettts_amd._handle import ptr

pytestmark = pytest.mark.gpu
OPB = _lib.AUDIO_OUT_PER_BLOCK
# L / M = 3/1, 1/2, 3/2, 441/160, 160/441
RATES = [(16000, 48000), (16000, 8000), (16000, 24000), (16000, 44100), (44100, 16000)]
IDS = ["3/1", "1/2", "3/2", "441/160", "160/441"]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def rs(dev):
    """One Resampler per pair of rates, shared by the module."""
    from viettts_amd.audio import Resampler

    made = {}

    def get(in_rate, out_rate):
        if (in_rate, out_rate) not in made:
            made[(in_rate, out_rate)] = Resampler(in_rate, out_rate, dev)
        return made[(in_rate, out_rate)]

    yield get
    for r in made.values():
        r.close()


@pytest.fixture(scope="module")
def inputs():
    """The three inputs of the parity tests, made once: speech-like with a noise floor, white noise, and the speech's PCM16 form."""
    rng = np.random.default_rng(2024)
    speech = oracle.speechlike(rng, 6000)
    noise = (0.25 * rng.standard_normal(2048)).astype(np.float32)
    pcm = np.rint(speech.astype(np.float64) * 32768.0).astype(np.int16)
    return {"speech": speech, "noise": noise, "pcm": pcm}


_REF = {}


def _reference(name, x, rates):
    """(fp64 oracle, err_ref32) of one input at one pair of rates, computed once per module run."""
    key = (name, rates)
    if key not in _REF:
        xf = x.astype(np.float32) / np.float32(32768.0) if x.dtype == np.int16 else x
        want = oracle.resample(xf, *rates)
        e32 = float(np.abs(oracle.resample(xf, *rates, dtype=np.float32).astype(np.float64) - want).max())
        _REF[key] = (want, e32)
    return _REF[key]


def _bar(err_ref32, want):
    return 4.0 * float(err_ref32) + 2.0 ** -22 * float(np.abs(want).max())


def _host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


@pytest.mark.parametrize("rates", RATES, ids=IDS)
@pytest.mark.parametrize("name", ["speech", "noise", "pcm"])
def test_parity_with_the_oracle(rs, inputs, rates, name):
    x = inputs[name]
    want, e32 = _reference(name, x, rates)
    got = _host(rs(*rates)(x))
    assert got.shape == want.shape and got.dtype == np.float32
    err, bar = float(np.abs(got.astype(np.float64) - want).max()), _bar(e32, want)
    print(f"\n{name} {rates[0]} -> {rates[1]}: max|gpu - fp64| = {err:.3e}, err_ref32 = {e32:.3e}, ratio {err / e32:.2f}, bar {bar:.3e}, max|y| {np.abs(want).max():.3f}")
    assert e32 > 0 and np.abs(want).max() > 0.1
    assert err <= bar


@pytest.mark.parametrize("rates", RATES, ids=IDS)
def test_rows_shorter_than_the_filter(rs, rates):
    rng = np.random.default_rng(7)
    r = rs(*rates)
    for S in (1, 2, 17):
        x = (0.5 * rng.standard_normal(S)).astype(np.float32)
        want = oracle.resample(x, *rates)
        e32 = float(np.abs(oracle.resample(x, *rates, dtype=np.float32).astype(np.float64) - want).max())
        got = _host(r(x))
        assert got.shape == want.shape == (r.out_samples(S),)
        assert np.abs(got.astype(np.float64) - want).max() <= _bar(e32, want), (S, rates)


@pytest.mark.parametrize("rates,sizes", [((16000, 8000), (2 * OPB - 2, 2 * OPB, 2 * OPB + 2)), ((16000, 48000), ((OPB - 1) // 3, (OPB - 1) // 3 + 1))],
                         ids=["1/2", "3/1"])
def test_output_counts_around_a_workgroups_tile(rs, rates, sizes):
    """1/2: rows of OPB - 1, OPB and OPB + 1 outputs; 3/1: OPB - 1 and OPB + 2, as one ragged batch (zeros past a row's own count) and
    each row alone."""
    rng = np.random.default_rng(8)
    r = rs(*rates)
    counts = [r.out_samples(S) for S in sizes]
    if rates == (16000, 8000):
        assert counts == [OPB - 1, OPB, OPB + 1]
    else:
        assert counts == [OPB - 1, OPB + 2]
    x = (0.3 * rng.standard_normal((len(sizes), max(sizes)))).astype(np.float32)
    got = _host(r(x, lengths=list(sizes)))
    assert got.shape == (len(sizes), max(counts))
    for b, (S, n) in enumerate(zip(sizes, counts)):
        want = oracle.resample(x[b, :S], *rates)
        e32 = float(np.abs(oracle.resample(x[b, :S], *rates, dtype=np.float32).astype(np.float64) - want).max())
        assert np.abs(got[b, :n].astype(np.float64) - want).max() <= _bar(e32, want), (b, S)
        assert np.all(got[b, n:] == 0), b
        assert np.array_equal(_host(r(x[b, :S].copy())), got[b, :n]), b


@pytest.mark.parametrize("rates", [(16000, 48000), (16000, 44100), (44100, 16000), (16000, 16000)], ids=["3/1", "441/160", "160/441", "1/1"])
def test_ragged_packed_and_pcm_input_are_the_same_bits(rs, dev, rates):
    lengths = [6000, 1, 385, 4097]
    rng = np.random.default_rng(9)
    pcm = rng.integers(-20000, 20000, size=(4, 6000), dtype=np.int16)
    xf = pcm.astype(np.float32) * np.float32(2.0 ** -15)
    r = rs(*rates)
    counts = r.out_lengths(lengths)
    strided = _host(r(xf, lengths=lengths))
    assert strided.shape == (4, max(counts))
    for b, (S, n) in enumerate(zip(lengths, counts)):
        alone = _host(r(xf[b, :S].copy()))
        assert alone.shape == (n,) and np.array_equal(strided[b, :n], alone), b  # the row is zero-extended at its OWN end
        assert np.all(strided[b, n:] == 0), b
    packed = _host(r(xf, lengths=lengths, packed=True))
    assert packed.shape == (sum(counts),)
    assert np.array_equal(packed, np.concatenate([strided[b, :n] for b, n in enumerate(counts)]))
    # PCM16 in is f32 in of pcm * 2^-15; an input whose rows are not 16-byte aligned (odd pitch) takes the scalar loads: same bits
    assert np.array_equal(_host(r(pcm, lengths=lengths)), strided)
    odd = torch.from_numpy(np.ascontiguousarray(np.pad(xf, ((0, 0), (0, 3))))).to(dev)
    assert np.array_equal(_host(r(odd, lengths=lengths)), strided)
    # PCM16 out, packed and strided
    p_str = _host(r(xf, lengths=lengths, out_dtype="pcm16"))
    p_pack = _host(r(xf, lengths=lengths, out_dtype="pcm16", packed=True))
    assert p_str.dtype == p_pack.dtype == np.int16
    assert np.array_equal(p_pack, np.concatenate([p_str[b, :n] for b, n in enumerate(counts)]))
    assert np.array_equal(p_str, wavio.float_to_pcm16(strided))
    if rates[0] == rates[1]:
        assert np.array_equal(strided[0], xf[0]) and np.array_equal(_host(r(pcm, out_dtype="pcm16")), pcm)  # the same format on both sides: copies
    else:
        assert np.array_equal(_host(r(pcm, lengths=lengths, out_dtype="pcm16")), p_str)


def _run_prefilled(r, x, lengths, out_dtype="f32", packed=False):
    """forward() through the C ABI into an output pre-filled with NaN (f32) or 12345 (PCM16): what no launch writes shows.  Packed outputs
    carry eight spare elements, which must keep the fill."""
    xt = torch.from_numpy(np.array(x)).to(r.device)  # (a copy: the shared rows are read-only)
    N, S = xt.shape
    outs = r.out_lengths(lengths)
    tdt, code, fill = (torch.int16, _lib.VTTS_AUDIO_PCM16, 12345) if out_dtype == "pcm16" else (torch.float32, _lib.VTTS_AUDIO_F32, float("nan"))
    out = torch.full((sum(outs) + 8,) if packed else (N, max(outs)), fill, dtype=tdt, device=r.device)
    if r._blob is None:
        r._pack()
    in_code = _lib.VTTS_AUDIO_PCM16 if xt.dtype == torch.int16 else _lib.VTTS_AUDIO_F32
    r._on_stream("forward", ptr(xt), in_code, N, S, (C.c_int32 * N)(*lengths), ptr(out), code, 0 if packed else max(outs))
    got = _host(out)
    if packed:
        assert np.all(got[-8:] == 12345) if out_dtype == "pcm16" else np.isnan(got[-8:]).all()
        got = got[:-8]
    return got


def test_rows_behind_the_launch_split_against_the_oracle(rs):
    """AUDIO_ROWS_PER_LAUNCH + 3 rows at 16 -> 24 kHz (tests/_row_split.py): the rows behind the split differ from the first rows in content
    and length and hold the longest row and an empty one.  Strided f32: every row against the fp64 oracle at the module's bar (once per
    distinct row), zeros past its count, and the rows at both ends of the split bit for bit the row alone.  Packed f32 is the strided rows
    back to back; PCM16 out, strided and packed, is float_to_pcm16 of them and within one step of the oracle's PCM, at most 1 % off it."""
    rates = (16000, 24000)
    bt = RS.audio_batch(_lib.AUDIO_ROWS_PER_LAUNCH)
    assert bt.N == _lib.AUDIO_ROWS_PER_LAUNCH + 3
    r = rs(*rates)
    counts = r.out_lengths(bt.lengths)

    def ref(row):
        if row.length == 0:
            return np.zeros(0), 0.0
        x = row.content[: row.length]
        want = oracle.resample(x, *rates)
        return want, float(np.abs(oracle.resample(x, *rates, dtype=np.float32).astype(np.float64) - want).max())

    refs = RS.per_kind(bt, ref)
    strided = _run_prefilled(r, bt.rows, bt.lengths)
    assert strided.shape == (bt.N, r.out_samples(max(bt.lengths[bt.P :]))) and not np.isnan(strided).any()
    worst = {False: 0.0, True: 0.0}
    for b, (n, (want, e32)) in enumerate(zip(counts, refs)):
        assert want.shape == (n,) and np.all(strided[b, n:] == 0), b
        if n:
            err, bar = float(np.abs(strided[b, :n].astype(np.float64) - want).max()), _bar(e32, want)
            worst[b >= bt.P] = max(worst[b >= bt.P], err / bar)
            assert err <= bar, (b, err, bar)
    for b in list(range(bt.k)) + list(bt.behind()):
        if counts[b]:
            assert np.array_equal(_host(r(bt.rows[b, : bt.lengths[b]].copy())), strided[b, : counts[b]]), b
    print(f"\naudio rows across the split: worst error / bar {worst[False]:.3f} before, {worst[True]:.3f} behind the split")
    flat = np.concatenate([strided[b, :n] for b, n in enumerate(counts)])
    assert np.array_equal(_run_prefilled(r, bt.rows, bt.lengths, packed=True).view(np.uint32), flat.view(np.uint32))
    p_str = _run_prefilled(r, bt.rows, bt.lengths, "pcm16")
    assert p_str.dtype == np.int16 and np.array_equal(p_str, wavio.float_to_pcm16(strided))
    assert np.array_equal(_run_prefilled(r, bt.rows, bt.lengths, "pcm16", packed=True), wavio.float_to_pcm16(flat))
    off = np.abs(wavio.float_to_pcm16(flat).astype(np.int32) - wavio.float_to_pcm16(np.concatenate([w for w, _ in refs])).astype(np.int32))
    print(f"PCM16 out: {100.0 * np.count_nonzero(off) / off.size:.3f} % of {off.size} samples differ from the oracle's PCM, max {off.max()} step")
    assert off.max() <= 1 and np.count_nonzero(off) <= 0.01 * off.size
    # the same batch at equal rates: copies of every row's own samples, through the same host loop
    same = _run_prefilled(rs(16000, 16000), bt.rows, bt.lengths)
    for b, n in enumerate(bt.lengths):
        assert np.array_equal(same[b, :n].view(np.uint32), bt.rows[b, :n].view(np.uint32)) and np.all(same[b, n:] == 0), b


def test_an_adopted_blob_gives_the_same_bits(rs, dev):
    """A second resampler that binds the first one's tap table (cloned) instead of packing its own."""
    from viettts_amd.audio import Resampler

    r = rs(16000, 44100)
    lengths = [1, 1000]
    x = torch.from_numpy(oracle.speechlike(np.random.default_rng(7), 2000).reshape(2, 1000)).to(dev)
    want = r(x, lengths, out_dtype="pcm16", packed=True)
    other = Resampler(16000, 44100, dev)
    try:
        other.adopt_packed(r.packed_blob().clone())
        got = other(x, lengths, out_dtype="pcm16", packed=True)
        torch.cuda.synchronize()
        assert got.dtype == torch.int16 and got.shape == (sum(r.out_lengths(lengths)),) and got.numel() > 2000
        assert torch.equal(got, want)
    finally:
        other.close()


def test_indices_past_2_to_31(rs, dev):
    """One row of 13 500 000 samples at 160/441: m M passes 2^31 at output 4 869 579.  Three windows of 2 048 outputs (start, across
    the crossing, end) against the oracle's windowed evaluation, at the parity tests' bar."""
    rates, S = (44100, 16000), 13_500_000
    L, M, _ = oracle.ratio(*rates)
    x = (0.25 * np.random.default_rng(10).standard_normal(S, dtype=np.float32)).astype(np.float32)
    r = rs(*rates)
    So = r.out_samples(S)
    assert So == oracle.out_samples(S, L, M) and (So - 1) * M > 2**31
    y = r(torch.from_numpy(x).to(dev))
    assert y.shape == (So,)
    cross = 2**31 // M
    for start in (0, cross - 1024, So - 2048):
        want = oracle.resample(x, *rates, start=start, count=2048)
        e32 = float(np.abs(oracle.resample(x, *rates, start=start, count=2048, dtype=np.float32).astype(np.float64) - want).max())
        got = _host(y[start : start + 2048])
        err = float(np.abs(got.astype(np.float64) - want).max())
        print(f"\noutputs {start} .. {start + 2047}: max|gpu - fp64| = {err:.3e}, err_ref32 = {e32:.3e}")
        assert np.abs(want).max() > 0.05
        assert err <= _bar(e32, want), start


def test_pcm16_conversion_is_float_to_pcm16(dev):
    from viettts_amd.audio import to_pcm16

    tiny = np.float32(1e-45)
    special = np.array([0.0, -0.0, 0.5, -0.5, 1.0, -1.0, 1.5, -1.5, 2.0 ** -15, -(2.0 ** -15), 2.0 ** -16, -(2.0 ** -16), tiny, -tiny, 1e-39, -1e-39,
                        0.5 / 32767, 1.5 / 32767, 2.5 / 32767, -0.5 / 32767, -1.5 / 32767, np.inf, -np.inf, 0.99999994, -0.99999994], dtype=np.float32)
    # exact ties of x * 32767 in double: x = (k + 0.5) / 32767 is not representable, but k + 0.5 = x * 32767 is for x = +-0.5 (16383.5)
    assert (np.float64(np.float32(0.5)) * 32767.0) % 1.0 == 0.5
    rng = np.random.default_rng(11)
    x = np.concatenate([special, rng.uniform(-1.2, 1.2, size=65536).astype(np.float32)])
    got = _host(to_pcm16(torch.from_numpy(x).to(dev)))
    want = wavio.float_to_pcm16(x)
    assert got.dtype == np.int16 and got.shape == want.shape
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:10]
    assert got[2] == 16384 and got[3] == -16384 and got[6] == 32767 and got[7] == -32767  # ties to even; clipped
    nan = _host(to_pcm16(torch.tensor([float("nan"), 0.25, -float("nan")], device=dev)))
    assert nan.tolist() == [0, int(wavio.float_to_pcm16(np.float32(0.25))), 0]
    # 2-D, ragged, packed
    m = rng.uniform(-1.2, 1.2, size=(3, 1500)).astype(np.float32)
    assert np.array_equal(_host(to_pcm16(m)), wavio.float_to_pcm16(m))
    assert np.array_equal(_host(to_pcm16(m, lengths=[1500, 7, 1025], packed=True)), wavio.float_to_pcm16(np.concatenate([m[0], m[1, :7], m[2, :1025]])))


@pytest.mark.parametrize("rates", RATES, ids=IDS)
def test_pcm16_out_after_resampling(rs, inputs, rates):
    """Every sample within one step of the oracle's PCM, and at most 1 % of the samples off it (the fp32 restatement alone is off in
    0.03 - 0.09 % on these inputs: a value within 1e-7 of a rounding boundary)."""
    for name in ("speech", "pcm"):
        x = inputs[name]
        want = wavio.float_to_pcm16(_reference(name, x, rates)[0]).astype(np.int32)
        got = _host(rs(*rates)(x, out_dtype="pcm16")).astype(np.int32)
        assert got.shape == want.shape
        off = np.abs(got - want)
        print(f"\n{name} {rates[0]} -> {rates[1]}: {100.0 * np.count_nonzero(off) / off.size:.3f} % of {off.size} samples differ, max {off.max()} step")
        assert off.max() <= 1
        assert np.count_nonzero(off) <= 0.01 * off.size


def test_argument_checks(rs, dev):
    r = rs(16000, 48000)
    x = torch.zeros((2, 64), device=dev)
    with pytest.raises(ValueError):
        r(x.double())
    with pytest.raises(ValueError):
        r(x.cpu())
    with pytest.raises(ValueError):
        r(x, out_dtype="f16")
    with pytest.raises(ValueError):
        r(x, lengths=[64])
    with pytest.raises(_lib.VttsError):
        r(x, lengths=[64, 65])
    assert _host(r(x, lengths=[0, 0])).shape == (2, 0) and _host(r(x, lengths=[0, 0], packed=True)).shape == (0,)
    assert np.all(_host(r(x)) == 0)


def test_resynthesis_from_another_rate(rs, dev):
    from viettts_amd.hifigan.config import V1
    from viettts_amd.hifigan.generator import Generator
    from viettts_amd.hifigan.synth import synthetic_params
    from viettts_amd.resynth import resynthesize

    gen = Generator(V1, device=dev)
    gen.load_params(synthetic_params(V1, 4321, "scaled"))
    try:
        rng = np.random.default_rng(12)
        w48 = torch.from_numpy(np.stack([oracle.speechlike(rng, 3 * 4096 + 5, 48000.0) for _ in range(2)])).to(dev)
        r = rs(48000, 16000)
        got = resynthesize(w48, gen, in_rate=48000).clone()
        want = resynthesize(r(w48), gen)
        torch.cuda.synchronize()
        assert got.shape == (2, 256 * 16) and torch.equal(got, want) and float(got.abs().max()) > 0
        lengths = [3 * 4096 + 5, 3 * 1000]
        got = resynthesize(w48, gen, lengths=lengths, in_rate=48000).clone()
        want = resynthesize(r(w48, lengths=lengths), gen, lengths=r.out_lengths(lengths))
        assert torch.equal(got, want)
        same = resynthesize(r(w48), gen, in_rate=16000)  # the model's own rate: nothing is converted
        assert torch.equal(same, resynthesize(r(w48), gen))
    finally:
        gen.close()


def test_pipeline_pcm16_and_output_rate(rs, dev):
    """Three sentences of the synthetic models the pipeline tests use: ``out_dtype="pcm16"`` is float_to_pcm16 of the default's
    output, and ``out_rate=48000`` is the resampler applied to the default's output."""
    from viettts_amd.hifigan.config import V1
    from viettts_amd.hifigan.generator import Generator
    from viettts_amd.hifigan.synth import synthetic_params
    from viettts_amd.nat.acoustic import AcousticModel
    from viettts_amd.nat.config import FLAGS
    from viettts_amd.nat.duration import DurationModel
    from viettts_amd.nat.synth import synthetic_acoustic_checkpoint, synthetic_duration_checkpoint
    from viettts_amd.pipeline import synthesize_sentences

    dm, am = DurationModel(device="cuda:0"), AcousticModel(device="cuda:0")
    dm.load_params(*synthetic_duration_checkpoint())
    am.load_params(*synthetic_acoustic_checkpoint())
    gen = Generator(V1, device="cuda:0", dtype="bf16")
    gen.load_params(synthetic_params(V1, 4321, "scaled"))
    try:
        rng = np.random.default_rng(41)
        sents = [[FLAGS.sil_index] + list(rng.integers(4, 90, size=int(rng.integers(2, 12)))) + [FLAGS.sil_index] for _ in range(3)]
        base = synthesize_sentences(sents, dm, am, gen, silence_duration=0.05)
        assert sorted(base) == [0, 1, 2] and all(base[i].dtype == np.float32 and base[i].shape[0] > 0 for i in base)
        base = {i: base[i].copy() for i in base}
        pcm = synthesize_sentences(sents, dm, am, gen, silence_duration=0.05, out_dtype="pcm16")
        for i in range(3):
            assert pcm[i].dtype == np.int16 and np.array_equal(pcm[i], wavio.float_to_pcm16(base[i])), i
        r = rs(16000, 48000)
        up = synthesize_sentences(sents, dm, am, gen, silence_duration=0.05, out_rate=48000)
        up16 = synthesize_sentences(sents, dm, am, gen, silence_duration=0.05, out_rate=48000, out_dtype="pcm16")
        for i in range(3):
            want = _host(r(base[i]))
            assert up[i].dtype == np.float32 and up[i].shape == (3 * base[i].shape[0],) and np.array_equal(up[i], want), i
            assert up16[i].dtype == np.int16 and np.array_equal(up16[i], wavio.float_to_pcm16(want)), i
        same = synthesize_sentences(sents, dm, am, gen, silence_duration=0.05, out_rate=16000)
        assert all(np.array_equal(same[i], base[i]) for i in range(3))
        with pytest.raises(ValueError):
            synthesize_sentences(sents, dm, am, gen, out_dtype="f16")
    finally:
        gen.close()
        dm.close()
        am.close()
