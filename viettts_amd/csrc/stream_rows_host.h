// The per-row bookkeeping every streamed session keeps on the host (limiter_stream.hip, resample_stream.hip), in plain C++ without HIP
// types: the cursors of each row, what a push is refused for (every refusal before any cursor moves) and how a launch's rows advance.
// Failures come back as audio_design.h's plan_rows reports them, a code and a text for the caller's failf.
// tools/check_stream_rows_host.cpp drives it against a brute-force model, stand-alone and under the sanitizers.
#pragma once

#include <stdint.h>

#include <cstdio>
#include <new>
#include <vector>

#include "../../include/vtts_hifigan.h"

namespace vtts_stream_rows {

struct Cursors {
    int rows = 0, max_chunk = 0;
    std::vector<int64_t> R, F;  // samples received, samples emitted
    std::vector<unsigned char> closed, parity;  // ended by a `last` push; which of the row's two device buffers the next push reads
    std::vector<unsigned> seen;  // the push that last named a row
    unsigned pushes = 0;

    // false = the host allocation failed
    bool init(int n_rows, int chunk) {
        rows = n_rows;
        max_chunk = chunk;
        try {
            R.assign(rows, 0);
            F.assign(rows, 0);
            closed.assign(rows, 0);
            parity.assign(rows, 0);
            seen.assign(rows, 0);
        } catch (const std::bad_alloc&) {
            return false;
        }
        return true;
    }

    bool has(int row) const { return row >= 0 && row < rows; }

    // A row starts over; its parity stays (either device buffer serves a row that has received nothing).
    void reset(int row) {
        R[row] = F[row] = 0;
        closed[row] = 0;
    }

    // A push of counts[i] samples onto rows[i], i < n: VTTS_OK, or the first refusal's code with `why` filled in.  No cursor changes.
    // A row may receive 2^31 - 1 - margin samples (margin = what the stage's tile arithmetic needs free, 0 = nothing).  Then hook(i, row,
    // count, why), the stage's own check of the row (0, or a code with why filled in): it runs per row so that the first bad row is the
    // one reported, whichever check it fails.
    template <typename Hook>
    int check_push(int n, const int32_t* rows_host, const int32_t* counts_host, int64_t c_stride, int margin, Hook&& hook, char (&why)[160]) {
        why[0] = 0;
        if (++pushes == 0) {  // (the counter wrapped: forget every earlier mark)
            seen.assign(seen.size(), 0u);
            pushes = 1;
        }
        const unsigned mark = pushes;
        auto refuse = [&](int code, const char* fmt, auto... args) {
            snprintf(why, sizeof why, fmt, args...);
            return code;
        };
        for (int i = 0; i < n; ++i) {
            const int r = rows_host[i];
            if (!has(r)) return refuse(VTTS_ERR_INVALID, "push: rows[%d] = %d is outside 0 .. %d", i, r, rows - 1);
            if (seen[r] == mark) return refuse(VTTS_ERR_INVALID, "push: row %d is named twice", r);
            seen[r] = mark;
            if (closed[r]) return refuse(VTTS_ERR_STATE, "push: row %d ended with its last push; reset() it first", r);
            const int64_t cnt = counts_host[i];
            if (cnt < 0 || cnt > max_chunk) return refuse(VTTS_ERR_INVALID, "push: counts[%d] = %lld is outside 0 .. max_chunk = %d", i, (long long)cnt, max_chunk);
            if (c_stride && cnt > c_stride) return refuse(VTTS_ERR_INVALID, "push: counts[%d] = %lld is above c_stride = %lld", i, (long long)cnt, (long long)c_stride);
            if (R[r] + cnt > 0x7fffffff - (int64_t)margin)
                return margin ? refuse(VTTS_ERR_SHAPE, "push: row %d would pass 2^31 - 1 - %d samples", r, margin)
                              : refuse(VTTS_ERR_SHAPE, "push: row %d would pass 2^31 - 1 samples", r);
            if (int rc = hook(i, r, cnt, why)) return rc;
        }
        return VTTS_OK;
    }
    int check_push(int n, const int32_t* rows_host, const int32_t* counts_host, int64_t c_stride, int margin, char (&why)[160]) {
        return check_push(n, rows_host, counts_host, c_stride, margin, [](int, int, int64_t, char (&)[160]) { return 0; }, why);
    }

    // After the launch that carried rows[0 .. n): each has taken counts[i] samples and given emitted[i]; last_host may be NULL (no row ends).
    void advance(int n, const int32_t* rows_host, const int32_t* counts_host, const int32_t* last_host, const int32_t* emitted) {
        for (int i = 0; i < n; ++i) {
            const int r = rows_host[i];
            F[r] += emitted[i];
            R[r] += counts_host[i];
            if (last_host && last_host[i])
                closed[r] = 1;
            else
                parity[r] ^= 1;
        }
    }
};

}  // namespace vtts_stream_rows
