"""The NAT duration and acoustic models on the GPU at every kind of model width vtts_nat_acoustic_create() accepts (tests/_nat_dims.py), against the
numpy oracles in fp64.  Every other NAT test runs encoder 256, decoder 512, prenet 256, mel 80, postnet 512 only.

The bar is tests/test_gpu_gta.py's rule, bar = min(4 * e32 + 2^-22 * max |want|, cap), with e32 = the oracle's own fp32 run against its fp64 run, the
largest over all cases of the width set (computed at test time, never from the library); cap = 5e-5 for the encoder, the teacher-forced pass and the
postnet, the existing 5e-4 * max(1, max |ref|) for the autoregressive mel, 2e-6 for durations.  tests/test_nat_dims_cpu.py shows on the oracles alone that
this bar admits the reference summed in another order (at most 0.22 of it) and sees a lost k-slice (2200 x it and more).  Every test prints err, e32, bar
and err / bar per quantity before it asserts (run with -s).  The tests allocate no output tensor themselves (the owners do); every
valid region is asserted finite, padded encoder rows exactly zero.

The kernels' index arithmetic at the sets S, O and X, walked by hand before the first run (viettts_amd/csrc/nat.hip; _nat_dims.geometry restates it):

* nat_dec_lstm_k / nat_tf_lstm_k, 8 waves, NIT = K / 8 iterations, NWMAX = ceil(NIT / 8) per wave, NAT_DEC_PD = 4 in flight.  Encoder LSTM at D = 64:
  K = 128, NIT = 16, NW = 2 < PD.  The prologue loads iterations it_lo .. it_lo + 3: the two beyond the wave's share are its neighbour's (in bounds) or
  clamped to NIT - 1 by load_it, and the loop leaves at j = NW, so they are loaded and never multiplied.  S decoder: K = 288 / 544, NIT = 36 / 68, NWMAX = 5 / 9:
  wave 7 gets NW = 1 / 5.  O: K = 352 / 608 -> NWMAX 6 / 10, wave 7 gets 2 / 6.  X: K = 1920 / 2944 -> 30 / 46 each.  Teacher-forced step: K = H / 2H.
* nat_conv_mfma_k / nat_conv_x3_k, 32-channel steps, float4 staging with cc = c + 4 <= Cin ? c : Cin - 4 (zeroed when c != cc).  Cin = 4 (S): one step, units
  c = 4 .. 28 re-read channel 0 .. 3 and store zeros.  Cin = 84 (O): 3 steps, the last holds 20 channels, c = 84 .. 92 clamp to 80.  Rows are Cin * 4 bytes =
  16 / 336, so every float4 is aligned.  Cout = 4 (S) / 36 (O): MB = 1 / 2 m-blocks, MR = 1, one grid row, waves 1 .. 3 (2, 3) own no block and only stage;
  the epilogue's `co >= Cout` drops lanes with 8 rq + 4 lh >= 4 (all but rq = 0, lh = 0) / in block 1 those past channel 36.  The packers zero-pad to
  32 x 32 (c < cin && co < cout).  The gate GEMMs have Cout = 4H >= 1024: MB >= 32, MR = 2, the only one-tap form nat_conv_x3_k is built for.
* nat_dec_proj_prenet_k, 1024 threads, 1024 / width chunks of per = roundup4(ceil(rows / chunks)) rows.  S (MEL 4, PN 32, H 256): projection 256 chunks x
  per 4 over 512 rows: chunks 128 .. 255 start at k >= rows and add zero; prenet 32 chunks x per 4 over 4 and 32 rows: 1 and 8 live.  part[] has 1024 slots
  and the highest index is chunks * width - 1 <= 1023.  O (84, 96): projection 12 chunks x per 44 (the last takes rows 484 .. 511), 16 idle threads; prenet
  10 chunks x per 12 over 84 and 96 rows (7 and 8 live), 64 idle threads.  X (128, 896, 1024): projection 8 x 256, prenet ONE chunk of 128 / 896 rows, 128
  idle threads.  Dynamic LDS (2H + 1024 + MEL + PN) * 16 bytes: S 25 152, O 27 456, W 45 056, X 65 536 = 64 KiB exactly, for which nat_dec_frames now raises
  the kernel's dynamic-LDS attribute as nat_cond_gates does for the mix (nothing at the other sets: below 48 KiB).
* nat_gates_mix_k: 4H / 1024 = 1 (S, O), 3 (W), 4 (X) column chunks per layer; LDS (roundup4(Lmax) + 16 Lmax) * 4 bytes: 48 KiB is passed at 723 tokens,
  54 400 at 800, 139 264 at 2048 (of the CU's 160 KiB).
* mask kernels: PN = 32 is half a 64-bit Threefry block (nat_keep_masks_k stops at `blk * 64 + j < PN`), 96 one and a half; the haiku kernel runs 64
  threads for 2 * PN = 64 values.
* what the walk found unservable: decoder widths that are no multiple of 256 (the mix's 1024-column chunks) — refused by create() now, they used to be
  accepted there and refused by every forward.

Figures so far (one MI355X run of this module: 39 passed), worst err / bar per width set, and for the worst case err | e32 | bar:

  quantity                    S      O      R      W      X     worst case
  encoder                   0.31   0.31   0.37   0.29   0.38   X (65, 129): 5.2e-7 | 3.0e-7 | 1.4e-6
  teacher-forced pre        0.74   0.35   0.44   0.60   0.66   S (2048, 40): 1.6e-6 | 4.5e-7 | 2.2e-6
  teacher-forced mel        0.75   0.31   0.40   0.54   0.60   S (65, 129): 1.8e-6 | 4.9e-7 | 2.4e-6
  postnet alone             0.23   0.57   0.73   0.53   0.71   R (63, 64): 2.5e-6 | 7.8e-7 | 3.4e-6
  autoregressive            0.39   0.28   0.50   0.26   0.36   R (65, 129): 2.7e-6 | 1.2e-6 | 5.3e-6
  autoregressive, masks     0.30   0.28   0.55   0.33   0.30   R (65, 129): 2.5e-6 | 1.0e-6 | 4.5e-6
  bf16x3 vs the oracle, err / cap   0.013  0.013  0.019  0.017  0.022;  vs the fp32 mode, of the range: 6.7e-6 (S, O: fallback), 9.2e-6 (R), 8.3e-6 (W), 1.05e-5 (X)
  duration model 64 / 128 / 192:    0.19 / 0.23 / 0.22 (err 5.1e-8, 1.4e-7, 4.1e-7)

(the long sentences (800, 40) and (2048, 40) are inside S's figures; every bit-equality, mask equality and refusal held; the 64 KiB projection step and the
136 KiB mix launched and agree with the oracle.)

What the first run found, and the fix: test_postnet_alone[W] (postnet 1024) lay OUTSIDE the bar, sentence (65, 129) at err 4.10e-6 | e32 9.26e-7 | bar 4.01e-6
(1.02; (64, 65) at 0.99).  No term was lost: nat_conv_mfma_k summed an output element as ONE fp32 fma chain, bias first, then 32-channel step -> tap ->
channel, 5 x 1024 = 5120 terms in the wide layers, and tools/restate_nat_conv_order.py, which restates that order on the CPU, gave 4.2e-6 for the chain alone
on the oracle's own fp32 `pre` where numpy's blocked fp32 sums are 8.3e-7: four to five times a blocked sum's error, and the bar allows four.  The kernel now
sets its running sums aside every 8 steps where a layer has more than 512 input channels (template flag FOLD; chains of 1280 terms, the parts added in step
order; up to 512 channels the instantiation, and so every bit and the speed, is the parent's).  The restatement of the folded order predicted 1.8e-6 (0.49 of
the bar); the GPU gives 2.13e-6 (0.53), and W's autoregressive figures fell from 0.63 / 0.75 to 0.26 / 0.33 with it.

Left unmeasured: long-form chunking and speed at other widths.  (The streaming session, the slot pool, forward_groups, forward_from_encoder and the
partitionable mask layout run at every set in tests/test_gpu_nat_sessions.py, bit for bit against the plain calls this module pins to the oracles.)
"""
import numpy as np
import pytest
import torch

import _gta_oracle as G
import _nat_dims as D
from oracle import nat_oracle as O
from viettts_amd._lib import VttsError

pytestmark = pytest.mark.gpu

SEEDED = tuple((L, F, 4000 + 10 * L + F) for L, F in D.ORDER_CASES)  # the dropout tests' sentences and their seeds
X3_SPLIT = {"S": False, "O": False, "R": True, "W": True, "X": True}
RNG_KEY = (123456789, 42)


@pytest.fixture(scope="module", params=D.GPU_ORDER)
def model(request):
    from viettts_amd.nat.acoustic import AcousticModel

    assert torch.cuda.is_available()
    sid = request.param
    m = AcousticModel(device="cuda:0", **D.dims(sid))
    m.load_params(*D.checkpoint(sid))
    yield sid, m
    m.close()


def _batch(sid, cases=D.CASES):
    cs = [D.case(sid, L, F) for L, F in cases]
    return cs, [c.tokens for c in cs], [c.dur for c in cs], [c.F for c in cs]


def _check(tag, got, want, e32, cap):
    assert got.shape == want.shape and got.dtype == np.float32 and np.isfinite(got).all(), tag
    err, b = D.report(tag, got, want, e32, cap)
    return err <= b


# ------------------------------------------------------------ per width set ------------------------------------------------------------
def test_encoder(model):
    sid, m = model
    cs, toks, _, _ = _batch(sid)
    enc = m.encode(toks)
    torch.cuda.synchronize()
    enc = enc.cpu().numpy()
    assert enc.shape == (len(cs), max(c.L for c in cs), 2 * D.dims(sid)["encoder_dim"])
    ok = []
    for i, c in enumerate(cs):
        ok.append(_check(f"{sid} encoder ({c.L}, {c.F})", enc[i, : c.L], D.oracle_encoder(sid, c.L, c.F), D.e32(sid, "enc"), D.CAP))
        assert not enc[i, c.L :].any()  # padded rows are exactly zero
    for i in (2, 7):
        assert np.array_equal(m.encode([toks[i]]).cpu().numpy()[0], enc[i, : cs[i].L]), i
    assert all(ok)


_TF = {}


def _teacher(sid, m):
    """One teacher-forced call per width set: the eight cases as one ragged batch with their own masks."""
    if sid not in _TF:
        cs, toks, durs, _ = _batch(sid)
        _TF[sid] = m.teacher_forced(toks, durs, [c.mels for c in cs], masks=([c.keep for c in cs], [c.zone for c in cs]), return_pre=True)
    return _TF[sid]


def test_teacher_forced(model):
    sid, m = model
    pre, mel = _teacher(sid, m)
    ok = []
    for i, (L, F) in enumerate(D.CASES):
        want = D.oracle_teacher(sid, L, F)
        ok.append(_check(f"{sid} teacher-forced pre ({L}, {F})", pre[i], want[0], D.e32(sid, "pre"), D.CAP))
        ok.append(_check(f"{sid} teacher-forced mel ({L}, {F})", mel[i], want[1], D.e32(sid, "mel"), D.CAP))
    assert all(ok)


def test_postnet_alone(model):
    """mel - pre of the teacher-forced call against the fp64 postnet of the GPU's OWN pre: the five K = 5 launches without the recurrence in front."""
    sid, m = model
    pre, mel = _teacher(sid, m)
    want = [D.postnet(sid, p) for p in pre]
    e32 = max(float(np.abs(D.postnet(sid, p, fp64=False).astype(np.float64) - w).max()) for p, w in zip(pre, want))
    ok = []
    for (L, F), p, y, w in zip(D.CASES, pre, mel, want):
        got = y.astype(np.float64) - p.astype(np.float64)
        assert np.isfinite(got).all()
        err, b = D.report(f"{sid} postnet residual ({L}, {F})", got, w, e32, D.CAP)
        ok.append(err <= b)
    assert all(ok)


def test_autoregressive_without_dropout(model):
    sid, m = model
    cs, toks, durs, nfs = _batch(sid)
    got = m(toks, durs, nfs)
    ok = []
    for c, g in zip(cs, got):
        want = D.oracle_ar(sid, c.L, c.F)
        ok.append(_check(f"{sid} autoregressive ({c.L}, {c.F})", g, want, D.e32(sid, "ar"), D.cap_ar(want)))
        assert np.array_equal(m([c.tokens], [c.dur], [c.F])[0], g), (c.L, c.F)  # a row does not depend on its batch
    assert all(ok)


def test_device_masks_and_autoregressive_with_them(model):
    sid, m = model
    PN, H = D.dims(sid)["prenet_dim"], D.dims(sid)["decoder_dim"]
    cs, toks, durs, nfs = _batch(sid, [(L, F) for L, F, _ in SEEDED])
    seeds = [sd for _, _, sd in SEEDED]
    keep = m.device_keep_masks(seeds + [2**40 + 17], max(nfs)).cpu().numpy()
    assert keep.shape == (4, max(nfs), 2, PN) and keep.dtype == np.uint8
    for i, sd in enumerate(seeds + [2**40 + 17]):
        assert np.array_equal(keep[i], O.threefry_keep_masks(sd, max(nfs), PN).astype(np.uint8)), sd
    hk = m.device_keep_masks_haiku(RNG_KEY, 3, 17, partitionable=False).cpu().numpy()
    want = O.haiku_prenet_keep_masks(np.array(RNG_KEY, dtype=np.uint32), 17, PN).astype(np.uint8)
    assert hk.shape == (3, 17, 2, PN) and all(np.array_equal(hk[b], want) for b in range(3))
    tk, tz = m.device_teacher_masks_haiku(RNG_KEY, 3, 17, partitionable=False)
    wk, wz = G.haiku_teacher_masks(RNG_KEY, 3, 17, PN, H)
    assert np.array_equal(tk.cpu().numpy(), wk.astype(np.uint8)) and np.array_equal(tz.cpu().numpy(), wz.astype(np.uint8))
    got = m(toks, durs, nfs, dropout_seeds=seeds)
    e32 = D.e32_ar_seeded(sid, SEEDED)
    ok = []
    for (L, F, sd), g in zip(SEEDED, got):
        want = D.oracle_ar(sid, L, F, True, sd)
        ok.append(_check(f"{sid} autoregressive, device masks ({L}, {F})", g, want, e32, D.cap_ar(want)))
        assert np.abs(g - D.oracle_ar(sid, L, F)).max() > 1e-3  # the masks matter
    assert all(ok)


def test_option_bf16x3(model):
    """tests/test_gpu_nat.py::test_acoustic_bf16x3_option's rules at this width set; S and O take the x3 gate GEMM and postnet around the fp32 step
    (their 16-row steps do not divide among 8 waves), R, W and X the split-state step."""
    sid, m = model
    PN, H = D.dims(sid)["prenet_dim"], D.dims(sid)["decoder_dim"]
    assert D.x3_split_state(PN, H) == X3_SPLIT[sid] == (((PN + H) // 16) % 8 == 0 and ((PN + 2 * H) // 16) % 8 == 0)
    cs, toks, durs, nfs = _batch(sid, [(L, F) for L, F, _ in SEEDED])
    seeds = [sd for _, _, sd in SEEDED]
    ref = m(toks, durs, nfs, dropout_seeds=seeds)
    assert m.get_option("bf16x3") == 0
    m.set_option("bf16x3", 1)
    try:
        got = m(toks, durs, nfs, dropout_seeds=seeds)
        alone = m([toks[1]], [durs[1]], [nfs[1]], dropout_seeds=[seeds[1]])[0]
    finally:
        m.set_option("bf16x3", 0)
    assert np.array_equal(alone, got[1])
    worst, ok = 0.0, []
    for (L, F, sd), g, r in zip(SEEDED, got, ref):
        assert np.isfinite(g).all()
        worst = max(worst, float(np.abs(g - r).max()) / max(1.0, float(np.abs(r).max())))
        want = D.oracle_ar(sid, L, F, True, sd)
        err = float(np.abs(g - want).max())
        print(f"[nat dims] {sid} bf16x3 ({L}, {F}): err {err:.3e}  cap {D.cap_ar(want):.3e}  err/cap {err / D.cap_ar(want):.3f}")
        ok.append(err < D.cap_ar(want))
    print(f"[nat dims] {sid} bf16x3 vs fp32 mode ({'split-state step' if X3_SPLIT[sid] else 'fp32 step, x3 GEMM and postnet'}): max |d mel| / range {worst:.2e}")
    assert 0.0 < worst < 2e-4 and all(ok)


# ------------------------------------------------------------ once, on S ------------------------------------------------------------
@pytest.fixture(scope="module")
def small():
    from viettts_amd.nat.acoustic import AcousticModel

    m = AcousticModel(device="cuda:0", **D.dims("S"))
    m.load_params(*D.checkpoint("S"))
    yield m
    m.close()


@pytest.mark.parametrize("B", [33, 65])
def test_wide_batch_rows_equal_rows_alone(small, B):
    """More than 32 sentences: two 32-sentence tiles per wave in the encoder's and the decoder's step kernels; 65 = a second 64-column block."""
    m = small
    cases = [D.CASES[(i + i // 8) % 8] for i in range(B)]
    cs, toks, durs, nfs = _batch("S", cases)
    got = m(toks, durs, nfs)
    for i in (0, 32, B - 1):
        assert np.array_equal(m([toks[i]], [durs[i]], [nfs[i]])[0], got[i]), i
    L, F = cases[32]
    want = D.oracle_ar("S", L, F)
    assert (L, F) == (9, 33) and _check(f"S autoregressive, row 32 of {B} ({L}, {F})", got[32], want, D.e32("S", "ar"), D.cap_ar(want))


@pytest.mark.parametrize("L, F", D.LONG_CASES)
def test_long_sentences(small, L, F):
    """Past 722 tokens the gate mix raises its dynamic-LDS attribute (54 KiB at 800 tokens, 136 KiB at the documented limit of 2048)."""
    m = small
    c = D.case("S", L, F)
    own = ((L, F),)
    e = {q: max(D.e32("S", q), D.e32("S", q, own)) for q in ("enc", "pre", "mel", "ar")}
    enc = m.encode([c.tokens]).cpu().numpy()[0]
    ok = [_check(f"S encoder ({L}, {F})", enc, D.oracle_encoder("S", L, F), e["enc"], D.CAP)]
    want = D.oracle_ar("S", L, F)
    ok.append(_check(f"S autoregressive ({L}, {F})", m([c.tokens], [c.dur], [F])[0], want, e["ar"], D.cap_ar(want)))
    pre, mel = m.teacher_forced([c.tokens], [c.dur], [c.mels], masks=([c.keep], [c.zone]), return_pre=True)
    want = D.oracle_teacher("S", L, F)
    ok.append(_check(f"S teacher-forced pre ({L}, {F})", pre[0], want[0], e["pre"], D.CAP))
    ok.append(_check(f"S teacher-forced mel ({L}, {F})", mel[0], want[1], e["mel"], D.CAP))
    assert all(ok)


def test_2049_tokens_are_refused_and_the_handle_still_works(small):
    m = small
    c = D.case("S", 9, 33)
    before = m([c.tokens], [c.dur], [c.F])[0]
    tok, dur = np.zeros(2049, np.int64), np.full(2049, 40.0 / 2049, np.float32)
    with pytest.raises(VttsError, match="2048"):
        m([tok], [dur], [40])
    with pytest.raises(VttsError, match="2048"):
        m.teacher_forced([tok], [dur], [np.zeros((40, 4), np.float32)])
    assert np.array_equal(m([c.tokens], [c.dur], [c.F])[0], before)


def test_resident_option_declines_other_widths(small):
    """The resident decoder is built for decoder 512 / prenet 256: with the option set, a call at other widths takes the per-frame launches."""
    m = small
    c = D.case("S", 9, 33)
    plain = m([c.tokens], [c.dur], [c.F])[0]
    m.set_option("resident", 1)
    try:
        got = m([c.tokens], [c.dur], [c.F])[0]
        assert not m.resident_used
    finally:
        m.set_option("resident", 0)
    assert np.array_equal(got, plain)


# ------------------------------------------------------------ duration model ------------------------------------------------------------
@pytest.mark.parametrize("dim", D.DURATION_WIDTHS)
def test_duration_model_widths(dim):
    from viettts_amd.nat.duration import DurationModel

    m = DurationModel(vocab_size=50, lstm_dim=dim, device="cuda:0")
    try:
        m.load_params(*D.duration_checkpoint(dim))
        sents = [D.duration_sentence(dim, L) for L in D.DURATION_LENGTHS]
        got = m(sents)
        ok = []
        for L, s, g in zip(D.DURATION_LENGTHS, sents, got):
            ok.append(_check(f"duration model {dim}, {L} tokens", g, D.duration_oracle(dim, L, True), D.duration_e32(dim), D.CAP_DURATION))
            assert np.array_equal(m([s])[0], g), L
        assert all(ok)
    finally:
        m.close()
