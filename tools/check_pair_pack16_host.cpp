// Host-only check of vtts::pair_g_pack16 (viettts_amd/csrc/vtts_internal.h): the weight order that resblock_pair_g_bf16_k's 16 x 16 x 32 loops read.
// For (C, K) = (64, 7), (64, 11), (128, 3) and (256, 11) it packs random weights into a buffer of exactly the old geometry's byte count (an overrun is the sanitizer's
// to report), then looks every (tap, ci, co) up where the fragment map says it is — [q = tap*(C/32) + ks][mblk16][lane][8], co = 16 mblk + (lane & 15),
// ci = 32 ks + 8 (lane >> 4) + e — and counts the elements visited: each exactly once.  Links nothing of the HIP runtime and needs no GPU:
//
//   clang++ -std=c++17 -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -fsanitize=address,undefined -fno-sanitize-recover=all \
//       tools/check_pair_pack16_host.cpp -o /tmp/check_pair_pack16_host && /tmp/check_pair_pack16_host
#include <cstdio>
#include <random>
#include <vector>

#include "../viettts_amd/csrc/vtts_internal.h"

static int check(int C, int K) {
    const size_t n = (size_t)K * C * C;
    const size_t old_bytes = vtts::bf16_packed_bytes(vtts::BPackGeom{C, C, C, K, C, 1});  // pair_g_pack_geom(C, K)
    int bad = 0;
    if (vtts::pair_g_pack16_bytes(C, K) != old_bytes || old_bytes != n * 2) {
        printf("C %d K %d: %zu bytes, the 32-block order has %zu\n", C, K, vtts::pair_g_pack16_bytes(C, K), old_bytes);
        return 1;
    }
    std::mt19937 rng(C * 100 + K);
    std::normal_distribution<float> nd(0.f, 1.f);
    std::vector<float> w(n);
    for (auto& v : w) v = nd(rng);
    std::vector<unsigned short> out(old_bytes / 2);
    vtts::pair_g_pack16(w.data(), C, K, out.data());
    std::vector<unsigned char> seen(n, 0);
    for (int tap = 0; tap < K; ++tap)
        for (int ci = 0; ci < C; ++ci)
            for (int co = 0; co < C; ++co) {
                const int ks = ci / 32, g = (ci % 32) / 8, e = ci % 8, mblk = co / 16, lane = 16 * g + co % 16;
                const size_t at = ((((size_t)tap * (C / 32) + ks) * (C / 16) + mblk) * 64 + lane) * 8 + e;
                if (at >= out.size() || seen[at]++) { ++bad; continue; }
                if (out[at] != vtts::f32_to_bf16_rne(w[((size_t)tap * C + ci) * C + co])) ++bad;
            }
    for (unsigned char s : seen) bad += s != 1;
    printf("C %3d K %2d: %zu elements, %zu bytes (= the 32-block order's), %d wrong\n", C, K, n, old_bytes, bad);
    return bad != 0;
}

int main() { return check(64, 7) | check(64, 11) | check(128, 3) | check(256, 11); }
