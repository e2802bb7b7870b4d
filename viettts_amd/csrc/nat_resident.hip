// The NAT acoustic decoder's frame loop as ONE resident kernel, for calls with 1 <= B <= 4 sentences (option "resident" of
// vtts_nat_acoustic_set_option, include/vtts_nat.h; the default stays nat.hip's three launches per frame).
//
// AcousticModel.inference's scan (vietTTS/nat/model.py:134-150) at batch 1 is a chain of dependent [1 x K] x [K x N] products: a frame costs
// kernel boundaries, not bytes.  Here one cooperative launch covers all Fmax frames.  A workgroup owns CW / 4 hidden units of BOTH LSTMs — all
// four gates of them — and copies its columns of the two recurrent matrices (Haiku rows [E, E + PN + H) and [E, E + PN + 2H): the conditioning's
// rows went into G1 / G2 ahead of the loop) into REGISTERS once, before frame 0: 16.8 MB over the grid, 64 floats per thread.  Cell states
// live in registers.  Nothing but the state vectors moves afterwards: at most 4 x 1664 floats per phase.
//
// Arithmetic (fp32, VALU fmaf, no matrix cores).  Every output element of every product is computed by one half-wave (32 lanes): lane `ks`
// walks k = ks, ks + 32, ks + 64, ... as one fmaf chain (lane 0's chain starts from the bias / the hoisted gates G, the others from 0), then the
// 32 partial sums meet in a five-level butterfly (xor 16, 8, 4, 2, 1).  That order does not depend on B, on the grid or on which workgroup
// holds the column: a row's result is the same bits alone or batched, on 64, 128 or 256 workgroups, run after run.
//
// Per frame five phases, each ended by a barrier across the grid:
//   LSTM 1  [p ; h1] -> h1'      LSTM 2  [p ; h1' ; h2] -> h2'      projection  [h1' ; h2'] -> mel_f (-> mel0[b][f])
//   prenet 1  mel_f -> p1        prenet 2  p1 -> p of frame f + 1   (relu, then x 2 * keep, as nat_dec_proj_prenet_k; the last frame stops after
//   the projection).  The projection's 80 and the prenet's 256 columns are spread one per workgroup (column c on workgroup c % grid).
//
// Exchange between workgroups (the XCDs' L2s are not coherent; cache-wide fences cost 32-51 us per sync on this chip,
// profiles/r04_e_nat_decoder_findings.md section 3): every exchanged value is written with an agent-scope relaxed atomic store (sc1: write-through), every
// storing wave waits vmcnt(0), the workgroup meets, ONE lane adds 1 to an agent-scope arrival counter and polls it with agent-scope atomic loads; the
// counter only grows (barrier n waits for n * grid; the host zeroes it on the stream before the launch).  Consumers read the payload ONLY with
// agent-scope atomic loads (sc1: past the CU's L1, which no other CU's store ever refreshes) into LDS.  Nothing depends on which XCD a workgroup runs on.
// Each exchanged vector is written in one phase, read in the next and not written again before four more barriers: single buffers suffice.
//
// Every spin is bounded: a wait longer than NAT_RES_BUDGET ticks of wall_clock64() (100 MHz: 100 ms, four orders of magnitude above a
// barrier) stores 1 into the abort word; every poll reads that word with the counter (one 8-byte load) and every workgroup that sees it
// leaves.  Frames not produced stay zero (the host cleared mel0 and the mel).  The launch is cooperative, so a grid that cannot be resident
// all at once is refused by the runtime instead of deadlocking.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "vtts_internal.h"

#ifndef VTTS_TIMELINE
#define VTTS_TIMELINE 0
#endif

namespace vtts {
namespace {

constexpr int RH = NAT_RES_H, RPN = NAT_RES_PN, RG4 = 4 * RH;
constexpr int RK1 = RPN + RH, RK2 = RPN + 2 * RH;  // state rows [p | h1] and [p | h1 | h2]
constexpr int RJ1 = RK1 / 32, RJ2 = RK2 / 32, RJP = 2 * RH / 32, RJF = RPN / 32, RJM = NAT_RES_MELMAX / 32;
// exchange buffer, in elements of 4 rows each: [mel | p1 | p | h1 | h2]
constexpr int XO_MEL = 0, XO_P1 = NAT_RES_MELMAX, XO_P = XO_P1 + RPN, XO_H1 = XO_P + RPN, XO_H2 = XO_H1 + RH;
static_assert(XO_H2 + RH == NAT_RES_XCH_ELEMS, "exchange layout");
constexpr unsigned long long NAT_RES_BUDGET = 10000000ull;  // wall_clock64() ticks of 10 ns

#define RES_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

template <int NB>
struct alignas(NB == 3 ? 4 : 4 * NB) ResRow {
    float v[NB];
};

__device__ __forceinline__ float res_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }

// the sum of a half-wave's 32 partial sums, the same tree on every lane
__device__ __forceinline__ float res_reduce32(float v) {
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// Barrier n of the launch across `grid` workgroups (target = n * grid).  false = the launch is being abandoned (this or another workgroup's
// wait ran out of its budget): the caller returns.
__device__ __forceinline__ bool res_grid_barrier(unsigned* sync, unsigned target, int* ok_lds) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's exchange stores have been written through
    __syncthreads();
    if (threadIdx.x == 0) {
        __hip_atomic_fetch_add(sync, 1u, RES_AGENT);
        const unsigned long long t0 = wall_clock64();
        int ok = 1;
        for (;;) {
            const unsigned long long v = __hip_atomic_load(reinterpret_cast<unsigned long long*>(sync), RES_AGENT);  // [arrivals | abort]
            if ((unsigned)(v >> 32) != 0u) {
                ok = 0;
                break;
            }
            if ((int)((unsigned)v - target) >= 0) break;
            if (wall_clock64() - t0 > NAT_RES_BUDGET) {
                __hip_atomic_store(sync + 1, 1u, RES_AGENT);
                ok = 0;
                break;
            }
            __builtin_amdgcn_s_sleep(1);
        }
        *ok_lds = ok;
    }
    __syncthreads();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");  // no instruction: the payload's loads stay behind the poll
    return *ok_lds != 0;
}

#if VTTS_TIMELINE
#define RES_TL(i)                                     \
    do {                                              \
        if (blockIdx.x == 0 && threadIdx.x == 0) {    \
            const unsigned long long n_ = wall_clock64(); \
            tl[i] += n_ - tl_last;                    \
            tl_last = n_;                             \
        }                                             \
    } while (0)
#else
#define RES_TL(i) \
    do {          \
    } while (0)
#endif

// NB = sentences, CW = gate columns per workgroup and layer (grid = 4H / CW workgroups of 32 * CW threads: a half-wave per column)
template <int NB, int CW>
__global__ __launch_bounds__(32 * CW) void nat_dec_resident_k(NatResidentArgs a) {
    constexpr int T = 32 * CW, NWG = RG4 / CW, UPW = CW / 4;
    __shared__ ResRow<NB> xs[RK2];              // [p | h1 | h2] of the sentences
    __shared__ ResRow<NB> ms[NAT_RES_MELMAX];   // the mel frame
    __shared__ ResRow<NB> p1s[RPN];             // the prenet's first layer
    __shared__ float gsum[CW][NB];              // gate pre-activations of the owned units
    __shared__ int ok_lds;
    const int t = threadIdx.x, ks = t & 31, cl = t >> 5, wg = blockIdx.x;
    const int Fmax = a.Fmax, MEL = a.MEL;
    // ---- this thread's share of the two recurrent matrices: column (gate, unit), rows ks + 32 j of the state order (Haiku rows E + ...)
    const int unit = wg * UPW + (cl >> 2), gate = cl & 3;
    float w1r[RJ1], w2r[RJ2];
    {
        const float* __restrict__ c1 = a.w1 + gate * RH + unit;
        const float* __restrict__ c2 = a.w2 + gate * RH + unit;
#pragma unroll
        for (int j = 0; j < RJ1; ++j) w1r[j] = c1[(size_t)(ks + 32 * j) * RG4];
#pragma unroll
        for (int j = 0; j < RJ2; ++j) w2r[j] = c2[(size_t)(ks + 32 * j) * RG4];
    }
    // G1 / G2 hold the gates in the step kernel's accumulator order (nat_model.h: nat_hcol)
    const int gcol = (unit >> 3) * 32 + (unit & 1) * 16 + ((unit >> 1) & 3) * 4 + gate;
    // the column of the projection / of the prenet this half-wave computes (clamped: a half-wave without one computes and stores nothing)
    const int ocol = wg + NWG * cl;
    const bool has_m = ocol < MEL, has_p = ocol < RPN;
    const int mcol = has_m ? ocol : MEL - 1, pcol = has_p ? ocol : RPN - 1;
    int nf[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) nf[b] = a.nframes[b];
    float cst1 = 0.0f, cst2 = 0.0f;  // cell states of (unit, sentence) = (t / NB, t % NB), threads [0, UPW * NB)
    for (int i = t; i < RK2 * NB; i += T) xs[i / NB].v[i % NB] = 0.0f;  // frame 0: p = prenet(0) = 0 (no biases), h1 = h2 = 0
    __syncthreads();
    unsigned epoch = 0;
#if VTTS_TIMELINE
    unsigned long long tl[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, tl_last = wall_clock64();
#endif
    // exchanged vector at element offset xo, n elements -> LDS rows
    auto fetch = [&](ResRow<NB>* dst, int xo, int n) {
        for (int i = t; i < n * NB; i += T) {
            const int k = i / NB, b = i % NB;
            dst[k].v[b] = __hip_atomic_load(a.xch + (size_t)(xo + k) * 4 + b, RES_AGENT);
        }
        __syncthreads();
    };
    // one LSTM layer's gates for the owned units from xs[0 .. 32 J), the cell update, h' -> exchange
    auto lstm = [&](const auto& wr, const float (&g0)[NB], float& cst, int xo, int f) {
        constexpr int J = std::extent<std::remove_reference_t<decltype(wr)>>::value;
        float acc[NB];
#pragma unroll
        for (int b = 0; b < NB; ++b) acc[b] = g0[b];
#pragma unroll
        for (int j = 0; j < J; ++j) {
            const ResRow<NB> x = xs[ks + 32 * j];
#pragma unroll
            for (int b = 0; b < NB; ++b) acc[b] = fmaf(wr[j], x.v[b], acc[b]);
        }
#pragma unroll
        for (int b = 0; b < NB; ++b) acc[b] = res_reduce32(acc[b]);
        if (ks == 0) {
#pragma unroll
            for (int b = 0; b < NB; ++b) gsum[cl][b] = acc[b];
        }
        __syncthreads();
        if (t < UPW * NB) {  // hk.LSTM: gates i, g, f, o; forget bias + 1
            const int ul = t / NB, b = t % NB;
            int nfb = nf[0];
#pragma unroll
            for (int q = 1; q < NB; ++q) nfb = b == q ? nf[q] : nfb;
            if (f < nfb) {
                const float gi = gsum[4 * ul + 0][b], gg = gsum[4 * ul + 1][b], gf = gsum[4 * ul + 2][b], go = gsum[4 * ul + 3][b];
                cst = res_sigmoid(gf + 1.0f) * cst + res_sigmoid(gi) * tanhf(gg);
                __hip_atomic_store(a.xch + (size_t)(xo + wg * UPW + ul) * 4 + b, res_sigmoid(go) * tanhf(cst), RES_AGENT);
            }
        }
    };
    for (int f = 0; f < Fmax; ++f) {
        // The projection's and the prenet's columns (44 floats per lane) are requested anew every frame, ahead of the barrier they would otherwise wait
        // behind (L1 / L2 hits under the wait): kept in registers beside the recurrent matrices' 64 they spill at 1024 threads per workgroup.  The
        // empty asm hides from the optimiser that the addresses are the same every frame.
        const float *wp = a.wp, *f1 = a.f1, *f2 = a.f2;
        int mo = ks * MEL + mcol, po = ks * RPN + pcol;  // (this lane's first row of its column)
        asm volatile("" : "+s"(wp), "+s"(f1), "+s"(f2), "+v"(mo), "+v"(po));
        // ---------------- LSTM 1: [p ; h1] -> h1' ----------------
        float g0[NB];
#pragma unroll
        for (int b = 0; b < NB; ++b) g0[b] = ks == 0 ? a.G1[((size_t)b * Fmax + f) * RG4 + gcol] : 0.0f;  // requested ahead of the wait
        if (f > 0) {
            if (!res_grid_barrier(a.sync, ++epoch * NWG, &ok_lds)) return;
            RES_TL(0);
            fetch(xs, XO_P, RPN);
        }
        lstm(w1r, g0, cst1, XO_H1, f);
        RES_TL(1);
        // ---------------- LSTM 2: [p ; h1' ; h2] -> h2' ----------------
#pragma unroll
        for (int b = 0; b < NB; ++b) g0[b] = ks == 0 ? a.G2[((size_t)b * Fmax + f) * RG4 + gcol] : 0.0f;
        if (!res_grid_barrier(a.sync, ++epoch * NWG, &ok_lds)) return;
        RES_TL(2);
        fetch(xs + RPN, XO_H1, RH);
        lstm(w2r, g0, cst2, XO_H2, f);
        RES_TL(3);
        // ---------------- projection: mel_f = [h1' ; h2'] @ wp + bp ----------------
        {
            float wr[RJP];
#pragma unroll
            for (int j = 0; j < RJP; ++j) wr[j] = wp[mo + 32 * j * MEL];  // this frame's weights on their way under the wait
            const float bias = ks == 0 ? a.bp[mcol] : 0.0f;
            if (!res_grid_barrier(a.sync, ++epoch * NWG, &ok_lds)) return;
            RES_TL(4);
            fetch(xs + RK1, XO_H2, RH);
            float acc[NB];
#pragma unroll
            for (int b = 0; b < NB; ++b) acc[b] = bias;
#pragma unroll
            for (int j = 0; j < RJP; ++j) {
                const ResRow<NB> x = xs[RPN + ks + 32 * j];
#pragma unroll
                for (int b = 0; b < NB; ++b) acc[b] = fmaf(x.v[b], wr[j], acc[b]);
            }
#pragma unroll
            for (int b = 0; b < NB; ++b) acc[b] = res_reduce32(acc[b]);
            if (ks == 0 && has_m) {
#pragma unroll
                for (int b = 0; b < NB; ++b)
                    if (f < nf[b]) {
                        a.mel0[((size_t)b * Fmax + f) * MEL + mcol] = acc[b];
                        __hip_atomic_store(a.xch + (size_t)(XO_MEL + mcol) * 4 + b, acc[b], RES_AGENT);
                    }
            }
            RES_TL(5);
        }
        if (f + 1 >= Fmax) break;
        // ---------------- prenet of frame f + 1: p1 = drop(relu(mel_f @ f1)), p = drop(relu(p1 @ f2)) ----------------
        auto dropout = [&](float v, unsigned char kp) {
            v = fmaxf(v, 0.0f);
            return a.keep ? (kp ? v * 2.0f : 0.0f) : v;
        };
        {
            float wr[RJM];
#pragma unroll
            for (int j = 0; j < RJM; ++j) wr[j] = ks + 32 * j < MEL ? f1[po + 32 * j * RPN] : 0.0f;
            unsigned char kp[NB];
#pragma unroll
            for (int b = 0; b < NB; ++b) kp[b] = a.keep ? a.keep[(((size_t)b * Fmax + f + 1) * 2 + 0) * RPN + pcol] : (unsigned char)1;
            if (!res_grid_barrier(a.sync, ++epoch * NWG, &ok_lds)) return;
            RES_TL(6);
            fetch(ms, XO_MEL, MEL);
            float acc[NB];
#pragma unroll
            for (int b = 0; b < NB; ++b) acc[b] = 0.0f;
#pragma unroll
            for (int j = 0; j < RJM; ++j) {
                if (ks + 32 * j < MEL) {
                    const ResRow<NB> x = ms[ks + 32 * j];
#pragma unroll
                    for (int b = 0; b < NB; ++b) acc[b] = fmaf(x.v[b], wr[j], acc[b]);
                }
            }
#pragma unroll
            for (int b = 0; b < NB; ++b) acc[b] = res_reduce32(acc[b]);
            if (ks == 0 && has_p) {
#pragma unroll
                for (int b = 0; b < NB; ++b)
                    if (f + 1 < nf[b]) __hip_atomic_store(a.xch + (size_t)(XO_P1 + pcol) * 4 + b, dropout(acc[b], kp[b]), RES_AGENT);
            }
            RES_TL(7);
        }
        {
            float wr[RJF];
#pragma unroll
            for (int j = 0; j < RJF; ++j) wr[j] = f2[po + 32 * j * RPN];
            unsigned char kp[NB];
#pragma unroll
            for (int b = 0; b < NB; ++b) kp[b] = a.keep ? a.keep[(((size_t)b * Fmax + f + 1) * 2 + 1) * RPN + pcol] : (unsigned char)1;
            if (!res_grid_barrier(a.sync, ++epoch * NWG, &ok_lds)) return;
            RES_TL(8);
            fetch(p1s, XO_P1, RPN);
            float acc[NB];
#pragma unroll
            for (int b = 0; b < NB; ++b) acc[b] = 0.0f;
#pragma unroll
            for (int j = 0; j < RJF; ++j) {
                const ResRow<NB> x = p1s[ks + 32 * j];
#pragma unroll
                for (int b = 0; b < NB; ++b) acc[b] = fmaf(x.v[b], wr[j], acc[b]);
            }
#pragma unroll
            for (int b = 0; b < NB; ++b) acc[b] = res_reduce32(acc[b]);
            if (ks == 0 && has_p) {
#pragma unroll
                for (int b = 0; b < NB; ++b)
                    if (f + 1 < nf[b]) __hip_atomic_store(a.xch + (size_t)(XO_P + pcol) * 4 + b, dropout(acc[b], kp[b]), RES_AGENT);
            }
            RES_TL(9);
        }
    }
#if VTTS_TIMELINE
    if (blockIdx.x == 0 && t == 0 && a.timeline)
        for (int i = 0; i < 10; ++i) a.timeline[i] = tl[i];
#endif
}

template <int CW>
hipError_t launch_cw(const NatResidentArgs& a, int B, hipStream_t s) {
    NatResidentArgs args = a;
    void* params[] = {&args};
    const void* fn = B == 1   ? reinterpret_cast<const void*>(&nat_dec_resident_k<1, CW>)
                     : B == 2 ? reinterpret_cast<const void*>(&nat_dec_resident_k<2, CW>)
                     : B == 3 ? reinterpret_cast<const void*>(&nat_dec_resident_k<3, CW>)
                              : reinterpret_cast<const void*>(&nat_dec_resident_k<4, CW>);
    return hipLaunchCooperativeKernel(fn, dim3(RG4 / CW), dim3(32 * CW), params, 0, s);
}

}  // namespace

hipError_t launch_nat_dec_resident(const NatResidentArgs& a, int B, int grid, hipStream_t s) {
    if (B < 1 || B > 4 || a.MEL < 4 || a.MEL > NAT_RES_MELMAX) return hipErrorInvalidValue;
    switch (grid) {
        case 64: return launch_cw<RG4 / 64>(a, B, s);
        case 128: return launch_cw<RG4 / 128>(a, B, s);
        case 256: return launch_cw<RG4 / 256>(a, B, s);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace vtts
