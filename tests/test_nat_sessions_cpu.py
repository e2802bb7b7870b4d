"""The cases of tests/test_gpu_nat_sessions.py reach what they are there for (tests/_nat_sessions.py), without a GPU: a later edit of the sentences,
chunks or pool plans that loses one of the paths below fails here instead of silently testing less."""
import _nat_dims as D
import _nat_sessions as N


def test_the_sentences_are_shared_with_the_width_tests_and_cover_the_row_ends():
    assert N.STREAM_CASES == ((1, 1), (2, 16), (9, 33), (64, 65), (65, 129)) and set(N.STREAM_CASES) <= set(D.CASES) and set(N.WIDE_CASES) <= set(D.CASES)
    assert (N.LMAX, N.FMAX) == (65, 129) and N.FMAX > 64 + N.HALO  # chunk 50: decode(60), then decode(110) crosses frame 64 inside one call
    assert len(set(N.seeds())) == len(N.STREAM_CASES) and all(N.seed(L, F) != N.seed(*c) for L, F in N.WIDE_CASES for c in N.STREAM_CASES if c != (L, F))
    frames = [F for _, F in N.STREAM_CASES]
    # chunk 32: a row that ends before the window [32, 64) (1, 16), inside its left halo (33), inside its right halo (65) and behind it (129)
    assert min(frames) < 32 - N.HALO and 32 - N.HALO <= 33 <= 32 + N.HALO and 64 <= 65 < 64 + N.HALO and max(frames) > 64 + N.HALO
    for sid in D.GPU_ORDER:
        toks, durs, nfs = N.batch(sid)
        assert nfs == frames and [len(t) for t in toks] == [L for L, _ in N.STREAM_CASES] == [len(d) for d in durs]


def test_window_units_take_1_21_20_and_32_float4():
    assert {sid: N.geometry(sid, 7, 5, 5)["C4"] for sid in "SORWX"} == {"S": 1, "O": 21, "R": 20, "W": 32, "X": 32}


def test_window_pitch_is_one_tile_for_chunks_1_7_32_and_two_for_50():
    assert {ch: N.geometry("W", ch, 5, 5)["W"] for ch in (1, 7, 32, 50)} == {1: 64, 7: 64, 32: 64, 50: 128}
    assert D.WIDTHS["W"][6] > 512  # the FOLD instantiation of nat_conv_mfma_k: layers with more than 512 input channels
    assert N.CHUNKS["R"] == N.CHUNKS["W"] == (1, 7, 32, 50) and all(set(N.CHUNKS[s]) == {7, 50} for s in "SOX") and set(N.CHUNKS) == set(D.GPU_ORDER)
    assert N.geometry("S", N.WIDE_MAX_WINDOW, N.WIDE_SLOTS, N.WIDE_SLOTS, N.WIDE_FMAX)["W"] == 64


def test_the_wide_pool_splits_its_list_and_takes_a_second_column_block():
    g = N.geometry("S", N.WIDE_MAX_WINDOW, N.WIDE_SLOTS, N.WIDE_SLOTS, N.WIDE_FMAX)
    assert g["list_launches"] == 2 and g["list_r0"] == (0, 48) and g["Bp"] == 128 and g["lgrid_y"] == 2
    assert N.geometry("S", 50, 5, 5)["lgrid_y"] == 1 and N.geometry("S", 50, 40, 4)["lgrid_y"] == 1 and N.geometry("S", 50, 40, 4)["list_r0"] == (0,)
    assert N.geometry("S", 8, 66, 48)["list_r0"] == (0,) and N.geometry("S", 8, 66, 49)["list_r0"] == (0, 48)


def test_the_wide_pools_finish_calls_are_what_the_issue_lists():
    calls = N.wide_finish_calls()
    n = [N.wide_case(s)[1] for s in range(N.WIDE_SLOTS)]
    assert [len(c) for c in calls[:3]] == [66, 48, 49] and all(len({s for s, _, _ in c}) == len(c) for c in calls)
    first = calls[0]
    assert [s for s, _, _ in first] == list(range(65, -1, -1)) and all(f0 == 0 for _, f0, _ in first)  # first windows; entry j is slot 65 - j
    assert {f1 for _, _, f1 in first} == {1, 3, 8} and any(f1 > n[s] for s, _, f1 in first)  # a width of 1; a window cut at the row's last frame
    # L.r0 = 0 in the second launch would hand list entry j the compact row of entry j + 48: every such pair is two different sentences
    for j in range(66 - 48):
        assert N.wide_case(first[j][0]) != N.wide_case(first[j + 48][0]), j
    assert all(f0 > 0 and f1 < n[s] for s, f0, f1 in calls[1])  # mid-row, nothing finishes: the 49 rows of the next call are all still open
    assert {f1 - f0 for _, f0, f1 in calls[1]} == {1, 2, 4} and any(f1 > n[s] for s, _, f1 in calls[2]) and any(f1 == n[s] for c in calls for s, _, f1 in c)
    # in order, contiguous, within max_window, and complete
    done = [0] * N.WIDE_SLOTS
    for c in calls:
        for s, f0, f1 in c:
            assert f0 == done[s] < n[s] and 0 < f1 - f0 <= N.WIDE_MAX_WINDOW
            done[s] = min(f1, n[s])
    assert done == n
    assert {N.wide_case(s) for s in range(N.WIDE_SLOTS)} == set(N.WIDE_CASES) and {N.wide_admit_tick(s) for s in range(N.WIDE_SLOTS)} == {0, 1, 4}
    assert all(N.wide_case(s) in N.WIDE_CASES for s in N.WIDE_ALONE) and max(n) == N.WIDE_FMAX and max(L for L, _ in N.WIDE_CASES) == N.WIDE_LMAX


def test_only_x_raises_the_projection_steps_lds_attribute():
    lds = {sid: N.geometry(sid, 50, 5, 5)["proj_lds_bytes"] for sid in D.GPU_ORDER}
    assert lds["X"] == 65536 > 48 * 1024 and all(lds[s] < 48 * 1024 for s in "SOR") and lds == {s: D.geometry(s)["proj_lds_bytes"] for s in D.GPU_ORDER}


def test_bf16x3_falls_back_to_the_fp32_step_at_exactly_s_and_o():
    assert {sid for sid in D.GPU_ORDER if not N.geometry(sid, 50, 5, 5)["x3_split_state"]} == {"S", "O"}


def test_both_layouts_of_the_pools_reset_clear_the_same_bytes():
    """Why no GPU test can tell which instantiation of nat_pool_reset_k pool_admit() picked: with ZW a multiple of 8 (prenet in multiples of 32, decoder
    in multiples of 256: every width create() accepts) the slot's eight rows in two bf16 planes ARE the bytes of its four-row fp32 groups, and both
    instantiations store zeros.  The choice that does show is nat_pool_ticks()'s, between the split-state and the fp32 STEP; the pool's bf16x3 cases run it."""
    for sid in D.GPU_ORDER:
        _, _, _, H, PN, _, _ = D.WIDTHS[sid]
        assert (PN + 2 * H) % 8 == 0
        for slots, slot in ((5, 0), (5, 4), (66, 33), (66, 65)):
            f32 = N.reset_bytes(sid, slots, slot, False)
            assert f32 == N.reset_bytes(sid, slots, slot, True) and len(f32) == 4 * (PN + 2 * H), (sid, slots, slot)
