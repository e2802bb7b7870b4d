// The rows of one launch and the host loop that cuts a call into launches, for every batched stage whose per-row lengths travel as kernel
// arguments.  Plain C++ without HIP types: the loop fills the launch's table; which pointers are re-based by r0, what is launched and how errors
// are reported stay with the stage.  tools/check_launch_rows_host.cpp drives it against a brute-force model, stand-alone under the sanitizers.
#pragma once

#include "../../include/vtts_hifigan.h"  // VTTS_OK, and <stdint.h>

namespace vtts_rows {

// The kernel-argument tables of a launch of up to R rows (their layout is the kernels' ABI: off before len).
template <int R>
struct Lens {
    int len[R];  // samples (or frames) of each row of this launch, 0 past its last row
};
template <int R>
struct OffLens {
    long long off[R];  // first output element of each row of this launch, from the call's output
    int len[R];
};

// fn(r0, nr, const Lens<R>&) for the launches r0 = 0, R, 2R .. of a call of N rows, nr = min(N - r0, R) rows each; lengths == NULL = every
// row has `full`.  The first non-zero return of fn ends the loop and is returned.
template <int R, typename Fn>
int for_each_launch(int N, const int32_t* lengths, int64_t full, Fn&& fn) {
    for (int r0 = 0; r0 < N; r0 += R) {
        const int nr = N - r0 < R ? N - r0 : R;
        Lens<R> rows;
        for (int b = 0; b < R; ++b) rows.len[b] = b < nr ? (lengths ? lengths[r0 + b] : (int)full) : 0;
        if (int rc = fn(r0, nr, rows)) return rc;
    }
    return VTTS_OK;
}

// The same with each row's first output element: (r0 + b) O_stride, or, packed (O_stride == 0), the output counts of all rows of the call
// before it, a row of len samples giving count(len).  The slots past the launch's last row keep counting (count(0) == 0): no kernel reads them.
template <int R, typename Count, typename Fn>
int for_each_launch_off(int N, const int32_t* lengths, int64_t full, int64_t O_stride, Count&& count, Fn&& fn) {
    long long packed = 0;
    for (int r0 = 0; r0 < N; r0 += R) {
        const int nr = N - r0 < R ? N - r0 : R;
        OffLens<R> rows;
        for (int b = 0; b < R; ++b) {
            rows.len[b] = b < nr ? (lengths ? lengths[r0 + b] : (int)full) : 0;
            rows.off[b] = O_stride ? (long long)(r0 + b) * O_stride : packed;
            packed += count(rows.len[b]);
        }
        if (int rc = fn(r0, nr, rows)) return rc;
    }
    return VTTS_OK;
}
template <int R, typename Fn>  // ... a row writes as many samples as it has
int for_each_launch_off(int N, const int32_t* lengths, int64_t full, int64_t O_stride, Fn&& fn) {
    return for_each_launch_off<R>(N, lengths, full, O_stride, [](int len) { return (long long)len; }, fn);
}

}  // namespace vtts_rows
