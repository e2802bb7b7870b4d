// Host-side engine behind the C ABI of include/vtts_hifigan.h.
//
// Holds the execution plan of the HiFi-GAN generator (vietTTS/hifigan/model.py:78-125): the 78
// convolution modules in execution order, where each one's weights live in the packed device blob,
// and the schedule that fuses LeakyReLU / bias / residual / MRF mean / tanh into the convolution
// kernels.  All device memory is caller-owned (blob, workspace, mel, wav).
#include "../../include/vtts_hifigan.h"

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "vtts_internal.h"

using namespace vtts;

namespace {

thread_local std::string g_last_error;

}  // namespace

int vtts::failf(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_last_error = buf;
    return code;
}

namespace {

enum Kind { KIND_CONV = 0, KIND_CONVT = 1 };

struct Layer {
    std::string key;
    int kind = KIND_CONV;
    int cin = 0, cout = 0, k = 0, dil = 1, stride = 1;
    int pad = 0;    // conv: symmetric pad, get_padding (model.py:8-10)
    int pad_a = 0;  // convT: left pad of the zero-stuffed input (lax "SAME")
    // host copies (Haiku layout)
    std::vector<float> w, b;
    bool have_w = false, have_b = false;
    // packed blob offsets in bytes
    size_t off_w = 0, off_b = 0, off_wp = 0;
    bool has_wp = false;
    size_t wp_floats = 0;
    // bf16 path: kernel class, packed bf16 weights, bias expanded to the GEMM's row count
    int bcls = BCLS_NONE;
    size_t off_wb = 0, wb_bytes = 0;
    int coutp = 0;  // GEMM rows: cout, or stride*cout for a transposed convolution run as Conv1d(k=3)
    // fused pair (this layer = convs1_z, next layer = convs2_z): [c1 slabs][c2 slabs] + [b1][b2]
    bool has_pair = false;
    size_t off_pw = 0, pw_bytes = 0, off_pb = 0;
    // whole ResBlock (this layer = convs1_0 of a ResBlock with a fused kernel): six convolutions' fragments + six biases
    bool has_rb = false;
    size_t off_rw = 0, rw_bytes = 0, off_rb = 0;
    // transposed convolution on the register-streamed kernel (kernels_bf16_up.hip): a second packing of the 3-tap form
    bool has_ug = false;
    size_t off_ug = 0, ug_bytes = 0;
    // VTTS_BF16X3: this ResBlock convolution's split weights, [hi fragments][lo fragments] (kernels_x3.hip: pair_x3_pack)
    bool has_x3 = false;
    size_t off_x3 = 0;
};

}  // namespace

struct vtts_hifigan {
    vtts_hifigan_cfg cfg;
    int device = 0;
    int dtype = VTTS_F32;
    bool x3 = false;                 // VTTS_BF16X3: dtype stays VTTS_F32 (the fp32 engine's layouts and schedule), the ResBlock pairs run on kernels_x3.hip
    int hop = 1;
    std::vector<Layer> layers;       // execution order
    int idx_pre = -1, idx_post = -1;
    std::vector<int> idx_ups;        // per stage
    std::vector<int> idx_res;        // [stage][kernel][z][convs1|convs2] flattened: base index of each resblock
    size_t blob_bytes = 0;
    char* blob = nullptr;            // bound device blob (caller-owned)
    // options
    int64_t opt_kernels = 0;         // 0 auto, 1 generic only
    int64_t opt_microbatch = 0;      // 0 auto
    int64_t opt_profile = 0;
    int cur_b0 = 0;                 // first utterance of the micro-batch being launched
    const int* cur_lens = nullptr;  // ragged forward in flight: valid mel frames per utterance (device) ...
    int cur_T = 0;                  // ... of the T allocated
    int64_t opt_tiles = 0;           // 0 auto, 1 wide, 2 narrow
    int64_t opt_fuse = 2;            // bf16: 0 one kernel per convolution, 1 fused pairs, 2 fused pairs + whole ResBlocks at C = 32
    int64_t opt_streams = 0;         // micro-batches in flight on separate HIP streams (1..4; 0 = the engines' default: 2 — auto_streams)
    int64_t opt_graph = 1;           // small launches: replay a captured hipGraph once the same buffers were seen twice (0 = always eager)
    struct GraphEntry {
        const void* mel = nullptr;
        void* wav = nullptr;
        void* ws = nullptr;
        int B = 0, T = 0, seen = 0;
        uint64_t epoch = 0, last_use = 0;
        hipGraph_t graph = nullptr;
        hipGraphExec_t exec = nullptr;
    };
    std::vector<GraphEntry> graphs;  // at most GRAPH_SLOTS, least recently used evicted
    hipStream_t cap_stream = nullptr; // launches are recorded on this stream, graphs are launched on the caller's
    uint64_t epoch = 0, use_clock = 0;  // epoch: bumped by everything a captured launch sequence bakes in (options, the weight blob)
    int64_t opt_zigzag = 1;          // consecutive launches walk the batch in alternating directions (see next_zrev)
    unsigned zrev_count = 0;
    int64_t opt_tail = 1;            // bf16: conv_post + tanh inside the generator's last pair launch (0 = the separate streaming kernel)
    int64_t opt_upfuse = 3;          // bf16: bit 0 / 1 = ups_2 / ups_3 inside the pair launch that ends the stage before it (up_fused_bf16)
    int64_t opt_chains = 1;          // small launches: the MRF's ResBlocks of a stage on parallel streams (0 = one after the other, 2 = always)
    hipEvent_t ev_chain[3] = {nullptr, nullptr, nullptr};  // bf16: ResBlock j's output is in the shared accumulator (orders the accumulating epilogues)
    hipStream_t side_streams[3] = {nullptr, nullptr, nullptr};
    hipEvent_t ev_fork = nullptr, ev_join[3] = {nullptr, nullptr, nullptr};
    // profiling of the dominant kernel class
    int prof_C = 0, prof_K = 0;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> prof_events;
    size_t prof_used = 0;
    double prof_flops = 0.0;
    std::string prof_name, prof_name_pair;
};

namespace {

int conv_same_pad_a(int k, int s) {
    // lax.conv_transpose padding="SAME": pad_len = k + s - 2; pad_a = k-1 if s > k-1 else ceil(pad_len/2)
    const int pad_len = k + s - 2;
    return (s > k - 1) ? (k - 1) : (pad_len + 1) / 2;
}

// option "profile" times the launches of one kernel class: the ResBlock (C, K) with the most FLOPs per mel frame, over the square
// convolutions after conv_pre (fp32 engines: those on the MFMA kernel); the first one in execution order wins a tie
void pick_dominant_class(vtts_hifigan* h, bool mfma_only) {
    double best_flops = -1.0;
    for (const Layer& l : h->layers) {
        if (&l == &h->layers[h->idx_pre] || l.kind != KIND_CONV || l.cin != l.cout || (mfma_only && !l.has_wp)) continue;
        double fl = 0.0;
        long len2 = 1;
        for (auto& m : h->layers) {
            if (m.kind == KIND_CONVT) len2 *= m.stride;
            if (m.kind == KIND_CONV && m.cin == l.cin && m.k == l.k && m.cin == m.cout) fl += 2.0 * len2 * m.cin * m.cout * m.k;
        }
        if (fl > best_flops) {
            best_flops = fl;
            h->prof_C = l.cin;
            h->prof_K = l.k;
        }
    }
}

bool dominant(const vtts_hifigan* h, const Layer& l) {
    return l.kind == KIND_CONV && l.cin == h->prof_C && l.cout == h->prof_C && l.k == h->prof_K;
}

int classify_bf16(const vtts_hifigan* h, const Layer& l, bool is_pre, bool is_post) {
    if (is_post) return (l.cin == 32 && l.cout == 1 && l.k == 7) ? BCLS_NONE - 1 : BCLS_NONE;  // -2 = streaming conv_post
    if (is_pre) return (l.cin <= 128 && l.cin % 8 == 0 && l.cout == 512 && l.k == 7) ? BCLS_PRE : BCLS_NONE;
    if (l.kind == KIND_CONVT) {
        if (!convT1d_f32_mfma_supported(l.cin, l.cout, l.k, l.stride, l.pad_a, 4)) return BCLS_NONE;  // same polyphase condition
        if (l.cin == 512) return BCLS_UP0;
        if (l.cin == 256) return BCLS_UP1;
        if (l.cin == 128) return BCLS_UP2;
        return BCLS_UP3;
    }
    if (l.cin != l.cout || !(l.k == 3 || l.k == 7 || l.k == 11) || l.dil > 5) return BCLS_NONE;
    switch (l.cin) {
        case 256: return BCLS_RES256;
        case 128: return BCLS_RES128;
        case 64: return BCLS_RES64;
        case 32: return BCLS_RES32;
    }
    return BCLS_NONE;
}

int build_layers_bf16(vtts_hifigan* h) {
    size_t off = 0;
    for (auto& l : h->layers) {
        const bool is_pre = (&l == &h->layers[h->idx_pre]), is_post = (&l == &h->layers[h->idx_post]);
        l.bcls = classify_bf16(h, l, is_pre, is_post);
        if (l.bcls == BCLS_NONE)
            return failf(VTTS_ERR_INVALID, "dtype bf16: no kernel for module %s (%d->%d, k=%d): the bf16 path covers the HiFi-GAN V1 shapes",
                         l.key.c_str(), l.cin, l.cout, l.k);
        l.coutp = (l.kind == KIND_CONVT) ? l.cout * l.stride : l.cout;
        l.off_b = off;
        off = align_up(off + (size_t)l.coutp * sizeof(float), 256);
        if (is_post) {
            l.off_w = off;
            off = align_up(off + (size_t)l.k * l.cin * l.cout * sizeof(float), 256);
        } else {
            const BPackGeom g = bf16_pack_geom(l.bcls, l.kind == KIND_CONVT ? 3 : l.k);
            l.wb_bytes = bf16_packed_bytes(g);
            l.off_wb = off;
            off = align_up(off + l.wb_bytes, 256);
            if (l.kind == KIND_CONVT || (is_pre && l.bcls == BCLS_PRE && l.cin == 80)) {  // the register-streamed kernel's packing (kernels_bf16_up.hip; its conv_pre tile is the 80-mel one)
                l.has_ug = true;
                l.ug_bytes = bf16_packed_bytes(convt_g_pack_geom(l.bcls));
                l.off_ug = off;
                off = align_up(off + l.ug_bytes, 256);
            }
        }
    }
    // (ResBlock2 generators, model.py:54-74, have no fused packings: their two convolutions per block run on the per-convolution kernel)
    for (size_t r = 0; r < h->idx_res.size() && h->cfg.resblock != 2; ++r) {
        for (int z = 0; z < 3; ++z) {
            Layer& c1 = h->layers[h->idx_res[r] + 2 * z];
            const Layer& c2 = h->layers[h->idx_res[r] + 2 * z + 1];
            if (!pair_bf16_supported(c1.cin, c1.k, c1.dil) || c2.dil != 1 || c2.k != c1.k) continue;
            c1.has_pair = true;
            c1.pw_bytes = 2 * bf16_packed_bytes(pair_g_pack_geom(c1.cin, c1.k));
            c1.off_pw = off;
            off = align_up(off + c1.pw_bytes, 256);
            c1.off_pb = off;
            off = align_up(off + (size_t)2 * c1.cin * sizeof(float), 256);
        }
    }
    for (size_t r = 0; r < h->idx_res.size() && h->cfg.resblock != 2; ++r) {
        Layer& c0 = h->layers[h->idx_res[r]];
        const int dils[3] = {h->layers[h->idx_res[r] + 0].dil, h->layers[h->idx_res[r] + 2].dil, h->layers[h->idx_res[r] + 4].dil};
        bool ok = resblock_bf16_supported(c0.cin, c0.k, dils);
        for (int q = 0; q < 6 && ok; ++q) {
            const Layer& l = h->layers[h->idx_res[r] + q];
            ok = l.cin == c0.cin && l.cout == c0.cin && l.k == c0.k && ((q & 1) ? l.dil == 1 : true);
        }
        if (!ok) continue;
        c0.has_rb = true;
        c0.rw_bytes = 6 * bf16_packed_bytes(pair_g_pack_geom(c0.cin, c0.k));
        c0.off_rw = off;
        off = align_up(off + c0.rw_bytes, 256);
        c0.off_rb = off;
        off = align_up(off + (size_t)6 * c0.cin * sizeof(float), 256);
    }
    h->blob_bytes = off;
    pick_dominant_class(h, false);
    for (auto& l : h->layers)
        if (dominant(h, l)) h->prof_name = bf16_kernel_name(l.bcls, l.k);
    h->prof_name_pair = pair_g_kernel_name(h->prof_C, h->prof_K);
    return VTTS_OK;
}

int build_layers(vtts_hifigan* h) {
    const vtts_hifigan_cfg& c = h->cfg;
    auto add = [&](const std::string& key, int kind, int cin, int cout, int k, int dil, int stride) {
        Layer l;
        l.key = key;
        l.kind = kind;
        l.cin = cin;
        l.cout = cout;
        l.k = k;
        l.dil = dil;
        l.stride = stride;
        if (kind == KIND_CONV) l.pad = (k * dil - dil) / 2;
        else l.pad_a = conv_same_pad_a(k, stride);
        h->layers.push_back(l);
        return (int)h->layers.size() - 1;
    };
    const int c0 = c.upsample_initial_channel;
    h->idx_pre = add("generator/~/conv1_d", KIND_CONV, c.num_mels, c0, 7, 1, 1);
    int n = 0;
    h->hop = 1;
    for (int i = 0; i < c.num_upsamples; ++i) {
        const int cin = c0 >> i, cout = c0 >> (i + 1);
        h->idx_ups.push_back(add("generator/~/ups_" + std::to_string(i), KIND_CONVT, cin, cout,
                                 c.upsample_kernel_sizes[i], 1, c.upsample_rates[i]));
        h->hop *= c.upsample_rates[i];
        for (int j = 0; j < c.num_kernels; ++j) {
            const std::string base = "generator/~/res_block1_" + std::to_string(n) + "/~/";
            int first = -1;
            if (c.resblock == 2) {
                // ResBlock2 (model.py:54-74): two convolutions, default hk.Conv1D names inside the module named res_block1_N (model.py:105)
                for (int z = 0; z < 2; ++z) {
                    int i1 = add(base + (z == 0 ? std::string("conv1_d") : "conv1_d_" + std::to_string(z)), KIND_CONV, cout, cout,
                                 c.resblock_kernel_sizes[j], c.resblock_dilation_sizes[j][z], 1);
                    if (z == 0) first = i1;
                }
                h->idx_res.push_back(first);  // layers first, first + 1
                ++n;
                continue;
            }
            for (int z = 0; z < 3; ++z) {
                int i1 = add(base + "convs1_" + std::to_string(z), KIND_CONV, cout, cout, c.resblock_kernel_sizes[j],
                             c.resblock_dilation_sizes[j][z], 1);
                add(base + "convs2_" + std::to_string(z), KIND_CONV, cout, cout, c.resblock_kernel_sizes[j], 1, 1);
                if (z == 0) first = i1;
            }
            h->idx_res.push_back(first);  // layers first..first+5 = c1_0, c2_0, c1_1, c2_1, c1_2, c2_2
            ++n;
        }
    }
    h->idx_post = add("generator/~/conv1_d_1", KIND_CONV, c0 >> c.num_upsamples, 1, 7, 1, 1);

    if (h->dtype == VTTS_BF16) return build_layers_bf16(h);

    // blob layout: per layer plain weights, bias, optional MFMA-packed weights; 256-B aligned
    size_t off = 0;
    for (auto& l : h->layers) {
        l.off_w = off;
        off = align_up(off + (size_t)l.k * l.cin * l.cout * sizeof(float), 256);
        l.off_b = off;
        off = align_up(off + (size_t)l.cout * sizeof(float), 256);
        const bool is_pre = (&l == &h->layers[h->idx_pre]);
        if (h->dtype == VTTS_F32 && l.kind == KIND_CONV && conv1d_f32_mfma_supported(l.cin, l.cout, l.k, l.dil, 4, is_pre)) {
            l.has_wp = true;
            l.wp_floats = conv1d_f32_mfma_packed_floats(l.cin, l.cout, l.k);
            l.off_wp = off;
            off = align_up(off + l.wp_floats * sizeof(float), 256);
        } else if (h->dtype == VTTS_F32 && l.kind == KIND_CONVT &&
                   convT1d_f32_mfma_supported(l.cin, l.cout, l.k, l.stride, l.pad_a, 4)) {
            l.has_wp = true;
            l.wp_floats = convT1d_f32_mfma_packed_floats(l.cin, l.cout, l.k);
            l.off_wp = off;
            off = align_up(off + l.wp_floats * sizeof(float), 256);
        }
    }
    if (h->x3) {
        Layer& pre = h->layers[h->idx_pre];
        if (conv_pre_x3_supported(pre.cin, pre.cout, pre.k, pre.dil)) {  // conv_pre on the split route too (round 5)
            pre.has_x3 = true;
            pre.off_x3 = off;
            off = align_up(off + conv_pre_x3_bytes(), 256);
        }
        for (int i : h->idx_ups) {
            Layer& l = h->layers[i];
            if (!convt_x3_supported(l.cin, l.cout, l.k, l.stride, l.pad_a, 4)) continue;
            l.has_x3 = true;
            l.off_x3 = off;
            off = align_up(off + convt_x3_bytes(l.cin, l.cout, l.stride), 256);
        }
    }
    if (h->x3 && h->cfg.resblock != 2) {
        for (size_t r = 0; r < h->idx_res.size(); ++r)
            for (int q = 0; q < 6; ++q) {
                Layer& l = h->layers[h->idx_res[r] + q];
                if (l.cin != l.cout || !pair_x3_supported(l.cin, l.k, l.dil, 4)) continue;
                l.has_x3 = true;
                l.off_x3 = off;
                off = align_up(off + pair_x3_conv_bytes(l.cin, l.k), 256);
            }
    }
    h->blob_bytes = off;
    pick_dominant_class(h, true);
    if (h->prof_C) h->prof_name = conv1d_f32_mfma_kernel_name(h->prof_C, h->prof_K);
    if (h->prof_C && h->x3) {
        char buf[96];
        snprintf(buf, sizeof(buf), "resblock_pair_x3_k<XTile<%d, %d,", h->prof_C, h->prof_K);
        h->prof_name = buf;
    }
    return VTTS_OK;
}

Layer* find_layer(vtts_hifigan* h, const char* key) {
    for (auto& l : h->layers)
        if (l.key == key) return &l;
    return nullptr;
}

// ---- one convolution launch -------------------------------------------------------------------
struct Act {  // channel-major activation view
    const float* p;
    long sb, sc, st;
};

// A launch's output (up to 1.07 GB at B = 64 x T = 1024) is the next launch's input, and the last 256 MB written are still in the Infinity
// Cache when that launch starts: walking the batch (blockIdx.z) in the opposite direction makes the consumer start with them instead of
// with the utterances written first, which have long been evicted (bf16 pass 40.00 -> 39.87 ms, three interleaved repetitions,
// gpurun_out/r03_exp40; the fp32 MFMA kernels take the same flag).  The samples do not depend on the order: utterances are independent.
int next_zrev(vtts_hifigan* h) { return h->opt_zigzag ? (int)(h->zrev_count++ & 1) : 0; }

// ragged batches (vtts_hifigan_forward_ragged): a layer whose input has L columns (fp32) / rows (bf16) per utterance slot learns each
// utterance's valid ones = frames * (columns per frame) (device_common.h: valid_len)
template <class Args>
void set_ragged(const vtts_hifigan* h, Args& a, int L) {
    a.lens = h->cur_lens ? h->cur_lens + h->cur_b0 : nullptr;
    a.len_mul = h->cur_lens ? L / h->cur_T : 1;
}

// Issues one launch of layer l's module (`launch` enqueues it on s) and reports its failure as "<what> for <module> failed".
// Option "profile": a launch of the dominant class that runs `convs` of its convolutions (0 = not timed) is bracketed by an event pair
// and credited with their ALGORITHMIC FLOPs (the bf16x3 kernels issue 3x as many bf16 MFMA FLOPs).
template <class Launch>
int launch_timed(vtts_hifigan* h, const Layer& l, int convs, int B, int L, hipStream_t s, const char* what, Launch launch) {
    const bool prof = convs > 0 && h->opt_profile && dominant(h, l);
    if (prof) {
        if (h->prof_used == h->prof_events.size()) {
            hipEvent_t e0, e1;
            HIP_TRY(hipEventCreate(&e0));
            HIP_TRY(hipEventCreate(&e1));
            h->prof_events.emplace_back(e0, e1);
        }
        HIP_TRY(hipEventRecord(h->prof_events[h->prof_used].first, s));
    }
    const hipError_t e = launch();
    if (e != hipSuccess) return failf(VTTS_ERR_HIP, "%s for %s failed: %s", what, l.key.c_str(), hipGetErrorString(e));
    if (prof) {
        HIP_TRY(hipEventRecord(h->prof_events[h->prof_used].second, s));
        h->prof_used++;
        h->prof_flops += convs * 2.0 * (double)B * L * l.cin * l.cout * l.k;
    }
    return VTTS_OK;
}

int run_layer(vtts_hifigan* h, const Layer& l, Act x, int B, int L, float slope_in, const float* res, float* y,
              int acc_mode, float div, int tanh_out, float* pre_act, hipStream_t s) {
    ConvArgs a;
    memset(&a, 0, sizeof(a));
    a.x = x.p;
    a.x_sb = x.sb;
    a.x_sc = x.sc;
    a.x_st = x.st;
    a.w = reinterpret_cast<const float*>(h->blob + l.off_w);
    a.wp = l.has_wp ? (h->blob + l.off_wp) : nullptr;
    a.bias = reinterpret_cast<const float*>(h->blob + l.off_b);
    a.res = res;
    a.y = y;
    a.B = B;
    a.Cin = l.cin;
    a.Cout = l.cout;
    a.K = l.k;
    a.dil = l.dil;
    a.pad = l.pad;
    a.stride = l.stride;
    a.pad_a = l.pad_a;
    a.L = L;
    a.Lout = (l.kind == KIND_CONVT) ? L * l.stride : L;
    a.slope_in = slope_in;
    a.acc_mode = acc_mode;
    a.div = div;
    a.tanh_out = tanh_out;
    a.pre_act = pre_act;
    a.tile_pref = (int)h->opt_tiles;
    a.zrev = next_zrev(h);
    set_ragged(h, a, L);

    hipError_t (*launch)(const ConvArgs&, hipStream_t) = launch_conv1d_generic;
    int timed = 0;
    const bool ncw = x.st == 1 && x.sc == L && (x.sb % 4) == 0;
    const bool want_mfma = h->opt_kernels == 0 && l.has_wp;
    if (l.kind == KIND_CONVT) {
        if (h->x3 && l.has_x3 && h->opt_kernels == 0 && h->opt_fuse >= 1 && ncw && !res && acc_mode == ACC_STORE) {
            a.wp = h->blob + l.off_x3;  // VTTS_BF16X3: the transposed convolutions on the bf16 matrix pipe with split operands too (kernels_x3.hip)
            launch = launch_convt_x3;
        } else if (want_mfma && ncw && !res && acc_mode == ACC_STORE && convT1d_f32_mfma_supported(l.cin, l.cout, l.k, l.stride, l.pad_a, L))
            launch = launch_convT1d_f32_mfma;
        else
            launch = launch_convT1d_generic;
    } else if (tanh_out) {
        if (h->opt_kernels == 0 && ncw && !res && acc_mode == ACC_STORE && conv_post_fast_supported(l.cin, l.cout, l.k, L))
            launch = launch_conv_post_fast;
    } else {
        const bool nwc = x.sc == 1 && x.st == l.cin;
        if (h->x3 && l.has_x3 && nwc && h->opt_kernels == 0 && h->opt_fuse >= 1 && !res && acc_mode == ACC_STORE && &l == &h->layers[h->idx_pre] &&
            (reinterpret_cast<uintptr_t>(x.p) & 15) == 0) {  // (float4 row loads: a mel pointer that is not 16-byte aligned takes the fp32 kernel)
            a.wp = h->blob + l.off_x3;  // VTTS_BF16X3: conv_pre with split operands (kernels_x3.hip: conv_pre_x3_k)
            launch = launch_conv_pre_x3;
        } else if (want_mfma && (ncw || nwc) && conv1d_f32_mfma_supported(l.cin, l.cout, l.k, l.dil, L, nwc)) {
            launch = launch_conv1d_f32_mfma;
            timed = 1;
        }
    }
    return launch_timed(h, l, timed, B, L, s, "kernel launch", [&] { return launch(a, s); });
}

// ---- ResBlock routes of the fp32 / bf16x3 engine --------------------------------------------------
// the fields every ResBlock launch shares: x [B][C][L] channel-major (rb[0]'s C and K) -> y with the MRF accumulate mode
ConvArgs resblock_args(vtts_hifigan* h, const Layer& c1, const float* x, int B, int L, float* y, int acc_mode, float div) {
    ConvArgs a;
    memset(&a, 0, sizeof(a));
    a.x = x;
    a.x_sb = (long)c1.cin * L;
    a.x_sc = L;
    a.x_st = 1;
    a.y = y;
    a.B = B;
    a.Cin = c1.cin;
    a.Cout = c1.cin;
    a.K = c1.k;
    a.stride = 1;
    a.L = L;
    a.Lout = L;
    a.slope_in = 0.1f;  // LRELU_SLOPE, both activations of every pair (model.py:46,48)
    a.acc_mode = acc_mode;
    a.div = div;
    a.zrev = next_zrev(h);
    set_ragged(h, a, L);
    return a;
}

// fp32 fused pair: c1 = convs1_z (rate d), c2 = convs2_z (rate 1) in one kernel (kernels_f32_pair.hip)
bool pair_f32_fusable(const Layer& c1, const Layer& c2, int L) {
    return c1.has_wp && c2.has_wp && c1.cin == c1.cout && c2.cin == c1.cin && c2.cout == c1.cin && c2.k == c1.k && c2.dil == 1 &&
           pair_f32_supported(c1.cin, c1.k, c1.dil, L);
}

bool pair_f32_wanted(const vtts_hifigan* h, const Layer& c1, const Layer& c2, int L) {
    if (h->opt_kernels != 0 || h->opt_fuse < 1 || !pair_f32_fusable(c1, c2, L)) return false;
    // Where the fused pair measured faster than the two launches it replaces (64 x 1024 frames, rocprofv3 per launch, gpurun_out/r04_run3):
    // C = 32: k = 3 / 7 / 11  -16 / -17 / -20 %;  C = 64: -13 / -6 / +-0 %;  C = 128: k = 3 -10 %, k = 7 -1 %, k = 11 +4.5 % (a fused pair
    // recomputes KS - 1 of every 128 columns and holds 78 KB of LDS: at C = 128, k = 11 that costs more than the saved traffic gains).
    // fuse = 1: C <= 64 only; fuse = 2 (default): + C = 128, k = 3; fuse = 3: every pair the kernel covers.
    return c1.cin <= 64 || (h->opt_fuse >= 2 && c1.cin == 128 && c1.k == 3) || h->opt_fuse >= 3;
}

// VTTS_BF16X3: the same pair on the bf16 matrix pipe with split operands (kernels_x3.hip); same buffers, same accumulate modes
bool pair_x3_wanted(const vtts_hifigan* h, const Layer& c1, const Layer& c2, int L) {
    return h->x3 && h->opt_kernels == 0 && h->opt_fuse >= 1 && c1.has_x3 && c2.has_x3 && c2.k == c1.k && c2.dil == 1 && c2.cin == c1.cin &&
           pair_x3_supported(c1.cin, c1.k, c1.dil, L);
}

// VTTS_BF16X3: where the whole-ResBlock kernel (kernels_x3_rb.hip) can run at all (vtts_hifigan_run_resblock takes it there whatever "fuse" says)
bool resblock_x3_runnable(const vtts_hifigan* h, const Layer* rb, int L) {
    if (!h->x3 || h->opt_kernels != 0) return false;
    for (int q = 0; q < 6; ++q)
        if (!rb[q].has_x3 || rb[q].cin != rb[0].cin || rb[q].cout != rb[0].cin || rb[q].k != rb[0].k || ((q & 1) && rb[q].dil != 1)) return false;
    const int dils[3] = {rb[0].dil, rb[2].dil, rb[4].dil};
    return resblock_x3_supported(rb[0].cin, rb[0].k, dils, L);
}

// VTTS_BF16X3: a whole ResBlock1 (three pairs + the MRF bookkeeping) in one launch where the kernel exists and is the faster choice
// (kernels_x3_rb.hip; fuse = 2: C = 32 and C = 64, k = 3; fuse = 3: wherever it exists); bit-identical to the three pair launches
bool resblock_x3_wanted(const vtts_hifigan* h, const Layer* rb, int L) {
    if (h->opt_fuse < 2 || !resblock_x3_runnable(h, rb, L)) return false;
    return h->opt_fuse >= 3 || resblock_x3_preferred(rb[0].cin, rb[0].k);
}

// how a ResBlock1's six convolutions (rb[0..5] = c1_0, c2_0, c1_1, c2_1, c1_2, c2_2) are launched; all routes give the same bits
enum Route { ROUTE_CONVS, ROUTE_PAIRS, ROUTE_RESBLOCK, ROUTE_X3_PAIRS, ROUTE_X3_RESBLOCK };

Route route_f32(const vtts_hifigan* h, const Layer* rb, int L) {
    if (resblock_x3_wanted(h, rb, L)) return ROUTE_X3_RESBLOCK;
    if (pair_x3_wanted(h, rb[0], rb[1], L) && pair_x3_wanted(h, rb[2], rb[3], L) && pair_x3_wanted(h, rb[4], rb[5], L)) return ROUTE_X3_PAIRS;
    if (pair_f32_wanted(h, rb[0], rb[1], L) && pair_f32_wanted(h, rb[2], rb[3], L) && pair_f32_wanted(h, rb[4], rb[5], L)) return ROUTE_PAIRS;
    return ROUTE_CONVS;
}

// one fused pair x' = c2(lrelu(c1(lrelu(x)))) + x on the fp32 kernel or (x3) the split-operand one
int run_pair_f32(vtts_hifigan* h, const Layer& c1, const Layer& c2, bool x3, const float* x, int B, int L, float* y, int acc_mode, float div,
                 hipStream_t s) {
    ConvArgs a = resblock_args(h, c1, x, B, L, y, acc_mode, div);
    a.bias = reinterpret_cast<const float*>(h->blob + c1.off_b);
    a.res = x;  // x = xt + x (model.py:50)
    a.dil = c1.dil;
    a.pad = c1.pad;
    const float* bias2 = reinterpret_cast<const float*>(h->blob + c2.off_b);
    if (x3)
        return launch_timed(h, c1, 2, B, L, s, "split-operand pair launch",
                            [&] { return launch_pair_x3(a, h->blob + c1.off_x3, h->blob + c2.off_x3, bias2, s); });
    a.wp = h->blob + c1.off_wp;
    return launch_timed(h, c1, 2, B, L, s, "fused fp32 pair launch", [&] { return launch_pair_f32(a, h->blob + c2.off_wp, bias2, s); });
}

int run_resblock_x3(vtts_hifigan* h, const Layer* rb, const float* x, int B, int L, float* y, int acc_mode, float div, hipStream_t s) {
    const ConvArgs a = resblock_args(h, rb[0], x, B, L, y, acc_mode, div);
    const int dils[3] = {rb[0].dil, rb[2].dil, rb[4].dil};
    const void* w[6];
    const float* bias[6];
    for (int q = 0; q < 6; ++q) {
        w[q] = h->blob + rb[q].off_x3;
        bias[q] = reinterpret_cast<const float*>(h->blob + rb[q].off_b);
    }
    // timed like the pair launches it replaces (six convolutions per launch)
    return launch_timed(h, rb[0], 6, B, L, s, "split-operand ResBlock launch", [&] { return launch_resblock_x3(a, dils, w, bias, s); });
}

// ---- bf16 path -------------------------------------------------------------------------------------
int run_layer_bf16(vtts_hifigan* h, const Layer& l, const void* x, int x_pitch, int cin_real, int B, int L, float slope_in,
                   float slope_out, const void* res, void* y, int acc_add, float div, hipStream_t s) {
    BConvArgs a;
    memset(&a, 0, sizeof(a));
    a.x = x;
    a.wp = h->blob + l.off_wb;
    a.bias = reinterpret_cast<const float*>(h->blob + l.off_b);
    a.res = res;
    a.y = y;
    a.B = B;
    a.L = L;
    set_ragged(h, a, L);
    a.x_pitch = x_pitch;
    a.cin_real = cin_real;
    a.dil = (l.kind == KIND_CONVT) ? 1 : l.dil;
    a.pad = (l.kind == KIND_CONVT) ? 1 : l.pad;
    a.convt_halves = (l.kind == KIND_CONVT) ? 1 : 0;
    a.slope_in = slope_in;
    a.slope_out = slope_out;
    a.acc_add = acc_add;
    a.div = div;
    const int K = (l.kind == KIND_CONVT) ? 3 : l.k;
    // transposed convolutions: the register-streamed kernel (fuse >= 1), else the first-generation 3-tap convolution.  Per launch at B = 64 x
    // T = 1024 (rocprofv3): ups_0 305 vs 422 us, ups_1 551 vs 985; ups_2 529 vs 688 and ups_3 422 vs 453 since round 3, when the two
    // HBM-bound ones (128 -> 2 x 64, 64 -> 2 x 32) got an LDS-staged epilogue that stores whole rows (round 2: 684 / 597 us with 32-byte
    // stores per frame and instruction, which is why they had stayed on the first-generation kernel; gpurun_out/r03_exp16).
    // conv_pre (80 -> 512, k = 7, fp32 mel in) runs on the same kernel since round 3 (7 taps per chunk, rows converted while staging)
    const bool ug = (l.kind == KIND_CONVT || l.bcls == BCLS_PRE) && l.has_ug && h->opt_fuse >= 1 && res == nullptr && acc_add == 0 && div == 1.0f;
    if (ug) a.wp = h->blob + l.off_ug;
    if (ug) a.zrev = next_zrev(h);
    return launch_timed(h, l, 1, B, L, s, "bf16 kernel launch",
                        [&] { return ug ? launch_convt_g_bf16(l.bcls, a, s) : launch_conv_bf16(l.bcls, K, a, s); });
}

// the fields every ResBlock launch of the bf16 engine shares: x [B][L][C] channels-last (rb[0]'s C) -> y, the consumer's activation
// and the MRF accumulate / mean in the epilogue
BConvArgs resblock_args_bf16(vtts_hifigan* h, const Layer& c1, const void* x, int B, int L, float slope_out, void* y, int acc_add, float div) {
    BConvArgs a;
    memset(&a, 0, sizeof(a));
    a.x = x;
    a.y = y;
    a.B = B;
    a.L = L;
    set_ragged(h, a, L);
    a.x_pitch = c1.cin;
    a.cin_real = c1.cin;
    a.slope_in = 0.1f;
    a.slope_out = slope_out;
    a.acc_add = acc_add;
    a.div = div;
    a.zrev = next_zrev(h);
    return a;
}

int run_pair_bf16(vtts_hifigan* h, const Layer& c1, const void* x, int B, int L, float slope_out, void* y, int acc_add, float div,
                  hipStream_t s, float* tail_wav = nullptr, const Layer* up = nullptr, void* up_y = nullptr) {
    BConvArgs a = resblock_args_bf16(h, c1, x, B, L, slope_out, y, acc_add, div);
    if (up) {  // the next stage's transposed convolution rides on this launch (kernels_bf16_rbg.hip: GUp): y is only read (the MRF accumulator), z = up(.) -> up_y
        a.up_wp = h->blob + up->off_ug;
        a.up_bias = reinterpret_cast<const float*>(h->blob + up->off_b);
        a.up_y = up_y;
    }
    a.wp = h->blob + c1.off_pw;
    a.bias = reinterpret_cast<const float*>(h->blob + c1.off_pb);
    a.dil = c1.dil;
    a.pad = c1.pad;
    a.tile_pref = (int)h->opt_tiles;
    if (tail_wav) {  // the stage-4 tail rides on this launch: conv_post + tanh from the rows this pair produces (kernels_bf16_rbg.hip: GTail)
        const Layer& post = h->layers[h->idx_post];
        a.tail_wav = tail_wav;
        a.tail_wf = reinterpret_cast<const float*>(h->blob + post.off_w);
        a.tail_bias = reinterpret_cast<const float*>(h->blob + post.off_b);
    }
    // (a launch that carries an upsampler is another kernel with other work: it is not timed as one of the dominant class's pair launches)
    return launch_timed(h, c1, up ? 0 : 2, B, L, s, "fused pair launch", [&] { return launch_pair_g_bf16(c1.cin, c1.k, a, s); });
}

int run_resblock_bf16(vtts_hifigan* h, const Layer* rb, const void* x, int B, int L, float slope_out, void* y, int acc_add, float div,
                      hipStream_t s) {
    BConvArgs a = resblock_args_bf16(h, rb[0], x, B, L, slope_out, y, acc_add, div);
    a.wp = h->blob + rb[0].off_rw;
    a.bias = reinterpret_cast<const float*>(h->blob + rb[0].off_rb);
    a.dils[0] = rb[0].dil;
    a.dils[1] = rb[2].dil;
    a.dils[2] = rb[4].dil;
    return launch_timed(h, rb[0], 0, B, L, s, "fused ResBlock launch", [&] { return launch_resblock_bf16(rb[0].cin, rb[0].k, a, s); });
}

Route route_bf16(const vtts_hifigan* h, const Layer* rb) {
    // the whole-ResBlock kernel where it exists and is the faster choice (fuse = 3: wherever it exists)
    if (h->opt_fuse >= 2 && rb[0].has_rb && (h->opt_fuse >= 3 || resblock_bf16_preferred(rb[0].cin, rb[0].k))) return ROUTE_RESBLOCK;
    if (h->opt_fuse >= 1 && rb[0].has_pair && rb[2].has_pair && rb[4].has_pair) return ROUTE_PAIRS;
    return ROUTE_CONVS;
}

// the stage-4 tail (option "tail", default on): the generator's last pair launch also runs conv_post + tanh on its own rows, so the stage
// output is never written and conv_post_bf16_k is not launched.  Where the last ResBlock runs as pairs and its last pair can carry it (V1:
// C = 32, k = 11); the caller also requires that nothing needs the stage output itself (no tap)
bool tail_fused_bf16(const vtts_hifigan* h) {
    if (!h->opt_tail || h->cfg.resblock == 2) return false;
    const Layer* rb = &h->layers[h->idx_res.back()];
    const Layer& post = h->layers[h->idx_post];
    return route_bf16(h, rb) == ROUTE_PAIRS && pair_tail_bf16_supported(rb[0].cin, rb[0].k, post.cin, post.cout, post.k);
}

// Option "upfuse" (bit 0: ups_2, bit 1: ups_3): the pair launch that ends stage i also runs ups_{i+1} on the rows its epilogue forms, writes the next
// stage's X and never writes stage i's output; upsample_bf16 is then skipped for stage i + 1.  Where the stage's last ResBlock runs as pairs and its
// last pair can carry that layer (V1: C = 128 / 64, k = 11, a stride-2 k = 4 transposed convolution to C / 2 channels on the register-streamed
// packing); the caller also requires that no tap needs stage i's output itself.  Otherwise the un-fused path runs, as with tail_fused_bf16.
bool up_fused_bf16(const vtts_hifigan* h, int i) {
    if (i < 1 || i > 2 || i + 1 >= h->cfg.num_upsamples || !((h->opt_upfuse >> (i - 1)) & 1) || h->cfg.resblock != 1 || h->opt_fuse < 1) return false;
    const int nk = h->cfg.num_kernels;
    const Layer* rb = &h->layers[h->idx_res[i * nk + nk - 1]];
    const Layer& up = h->layers[h->idx_ups[i + 1]];
    return route_bf16(h, rb) == ROUTE_PAIRS && up.has_ug &&
           pair_up_bf16_supported(rb[0].cin, rb[0].k, up.bcls, up.cin, up.cout, up.k, up.stride);
}

// ---- the pass plan: micro-batches, streams, workspace -------------------------------------------------------
size_t elem_bytes(const vtts_hifigan* h) { return h->dtype == VTTS_BF16 ? 2 : sizeof(float); }

size_t max_act_elems(const vtts_hifigan* h, int T) {
    // largest [C][L] activation per utterance over all stages (8192*T for V1)
    size_t best = (size_t)h->cfg.upsample_initial_channel * T;
    long L = T;
    for (int i = 0; i < h->cfg.num_upsamples; ++i) {
        L *= h->cfg.upsample_rates[i];
        size_t e = (size_t)(h->cfg.upsample_initial_channel >> (i + 1)) * L;
        if (e > best) best = e;
    }
    return best;
}

// Both engines run a large batch as two half-size passes on two streams: one pass's launch tails and memory phases lie under the other's
// MFMAs (fp32: 64 x 1024 frames 366.5 -> 363.9 ms, gpurun_out/r03_exp35; bf16 with the zigzag batch order: 39.95 -> 39.32-39.50 ms,
// profiles/r03_c_narrow_stage_findings.md §4, r03_exp42).  Micro-batches are independent, so the samples do not depend on the schedule
// (bit-identical: tests/test_gpu_bf16.py::test_ragged_batch_across_micro_batches_and_streams, test_gpu_parity.py).  A kernel's duration is its
// own only while nothing else shares the GPU: bench.py therefore times the dominant kernel in a one-stream calibration pass of the same build
// and inputs (option streams = 1), and tools/profile_final.sh profiles that schedule.
int auto_streams(const vtts_hifigan* h) { return h->opt_streams > 0 ? (int)h->opt_streams : 2; }

// mel frames per CALL the Python schedulers build their batches for (option "pass_frames": viettts_amd/longform.py, pipeline.py).  The bf16
// engine takes 65536 frames per call and cuts them into its micro-batches itself; the fp32 engine's callers hand it one micro-batch at a time.
int pass_frames(const vtts_hifigan* h) { return (h->dtype == VTTS_F32 && auto_streams(h) >= 2) ? 32768 : 65536; }

// mel frames per micro-batch (one sequence of launches on one stream)
int microbatch_frames(const vtts_hifigan* h) { return auto_streams(h) >= 2 ? 32768 : 65536; }

int pick_microbatch(const vtts_hifigan* h, int B, int T) {
    if (h->opt_microbatch > 0) return (int)std::min<int64_t>(h->opt_microbatch, B);
    // Enough frames per pass that every launch is many rounds of workgroups on the 256 CUs: with few
    // rounds the last, partly filled one costs 10-20 % (measured: bf16 61.6 ms/step at 4096 frames per
    // pass, 49.9 ms at 65536).  fp32 tiles are 2-4x narrower, so fewer frames reach the same round count.
    // (round 3: the fp32 engine too — 16384 frames per pass measured 388.4 ms per 64 x 1024 batch, 65536 frames 380.7 ms; the 8.6 GB of workspace are 3 % of the HBM)
    const int frames = microbatch_frames(h);
    int mb = (frames + T - 1) / T;
    if (mb < 1) mb = 1;
    if (mb > B) mb = B;
    // equal micro-batches, as many as a multiple of the streams (48 utterances of 1024 frames: 24 + 24, not 32 + 16; 256 sentences padded to
    // 281 frames: 4 x 64, not 3 x 86 on two streams): the streams finish together
    int nmb = (B + mb - 1) / mb;
    const int ns = auto_streams(h);
    if (nmb > 1 && ns > 1) nmb = (nmb + ns - 1) / ns * ns;
    if (nmb > B) nmb = B;
    mb = (B + nmb - 1) / nmb;
    return mb;
}

// The kernels may form one utterance's row * channel offsets (elements or bytes) in 32 bits and index the batch with
// blockIdx.z: a longer utterance goes through the chunk scheduler (viettts_amd/longform.py: 13-frame halo), a larger batch in
// several calls.
int check_pass_size(const vtts_hifigan* h, int B, int T) {
    const size_t bytes = max_act_elems(h, T) * elem_bytes(h);
    if (bytes >= ((size_t)1 << 31))
        return failf(VTTS_ERR_INVALID, "T=%d frames is too long for one pass (%zu activation bytes per utterance, limit 2^31): synthesize it in chunks",
                     T, bytes);
    if (pick_microbatch(h, B, T) > 65535) return failf(VTTS_ERR_INVALID, "at most 65535 utterances per pass (got %d)", B);
    return VTTS_OK;
}

// A single small micro-batch leaves most of the chip idle (B = 1 x T = 512: 256 workgroups of 4 waves in stage 1), and the MRF's
// ResBlocks of a stage are independent given the stage input: they then run on parallel streams (3 forwards in flight measured 2.2x the
// time of one: 1.36x the throughput).
constexpr int PAR_CHAIN_FRAMES = 2048;

// one micro-batch's buffers: X the stage input (ups output), S the MRF accumulator / stage output; ResBlock j's scratch T[j] (xt inside a
// pair), C[j] (the running x inside the ResBlock) and, fp32 parallel chains only, Y[j] (its separate output)
struct PassBufs {
    char *X = nullptr, *S = nullptr;
    char *T[VTTS_MAX_KERNELS] = {}, *C[VTTS_MAX_KERNELS] = {}, *Y[VTTS_MAX_KERNELS] = {};
};

// How a forward of B x T frames runs: micro-batches of mb utterances rotate over nstr streams, each in a workspace slot of its own.
// A slot holds nbuf buffers of `per` bytes (the widest stage's [C][L] activation of mb utterances):
//   ResBlocks one after the other: X | T | C | S (every ResBlock uses the same T, C)
//   parallel chains (one micro-batch, one slot): X | S | (T, C[, Y]) per ResBlock — fp32 / bf16x3: 2 + 3 * num_kernels, bf16: 2 + 2 * num_kernels
struct PassPlan {
    int mb = 1, nstr = 1, nbuf = 4;
    size_t es = 0, per = 0;
    bool par = false;
    int chain_bufs = 0;  // buffers per parallel chain

    size_t bytes() const { return (size_t)nstr * nbuf * per; }
    PassBufs buffers(void* ws, int si, int nk) const {
        char* slot = static_cast<char*>(ws) + (size_t)si * nbuf * per;
        auto at = [&](int q) { return slot + (size_t)q * per; };
        PassBufs b;
        b.X = at(0);
        b.S = at(par ? 1 : 3);
        for (int j = 0; j < nk; ++j) {
            b.T[j] = par ? at(2 + chain_bufs * j) : at(1);
            b.C[j] = par ? at(3 + chain_bufs * j) : at(2);
            if (par && chain_bufs == 3) b.Y[j] = at(4 + 3 * j);
        }
        return b;
    }
};

PassPlan plan_pass(const vtts_hifigan* h, int B, int T) {
    PassPlan p;
    p.mb = pick_microbatch(h, B, T);
    // Micro-batches are independent, so consecutive ones may run on different HIP streams: workgroups of
    // one micro-batch in an HBM phase (tile staging / epilogue) then share the CUs with workgroups of
    // another in its MFMA phase instead of every workgroup on the chip hitting HBM at the same time.
    const int nmb = (B + p.mb - 1) / p.mb;
    p.nstr = std::max(1, std::min(auto_streams(h), nmb));
    p.es = elem_bytes(h);
    p.per = align_up(max_act_elems(h, T) * (size_t)p.mb * p.es, 256);
    const int nk = h->cfg.num_kernels;
    if (h->opt_chains && ((long)B * T <= PAR_CHAIN_FRAMES || h->opt_chains == 2) && p.mb >= B)
        p.par = h->dtype == VTTS_F32 ? (nk == 2 || nk == 3) : (nk == 3 && h->cfg.resblock != 2);
    if (p.par) {
        p.chain_bufs = h->dtype == VTTS_F32 ? 3 : 2;
        p.nbuf = 2 + p.chain_bufs * nk;
    }
    return p;
}

int fork_streams(vtts_hifigan* h, int n, hipStream_t s, hipStream_t* out) {
    out[0] = s;
    if (n <= 1) return VTTS_OK;
    if (!h->ev_fork) {
        HIP_TRY(hipEventCreateWithFlags(&h->ev_fork, hipEventDisableTiming));
        for (int i = 0; i < 3; ++i) {
            HIP_TRY(hipStreamCreateWithFlags(&h->side_streams[i], hipStreamNonBlocking));
            HIP_TRY(hipEventCreateWithFlags(&h->ev_join[i], hipEventDisableTiming));
        }
    }
    HIP_TRY(hipEventRecord(h->ev_fork, s));
    for (int i = 1; i < n; ++i) {
        HIP_TRY(hipStreamWaitEvent(h->side_streams[i - 1], h->ev_fork, 0));
        out[i] = h->side_streams[i - 1];
    }
    return VTTS_OK;
}

int join_streams(vtts_hifigan* h, int n, hipStream_t s) {
    for (int i = 1; i < n; ++i) {
        HIP_TRY(hipEventRecord(h->ev_join[i - 1], h->side_streams[i - 1]));
        HIP_TRY(hipStreamWaitEvent(s, h->ev_join[i - 1], 0));
    }
    return VTTS_OK;
}

// runs chain(j, stream) for the nk ResBlocks of a stage on streams forked from s.  The streams are joined back into s whatever
// happens: during a graph capture an un-joined fork invalidates the capture
template <class Chain>
int run_chains_parallel(vtts_hifigan* h, int nk, hipStream_t s, Chain chain) {
    hipStream_t cs[4];
    int rc = fork_streams(h, nk, s, cs);
    for (int j = 0; j < nk && !rc; ++j) rc = chain(j, cs[j]);
    const int rj = join_streams(h, nk, s);
    return rc ? rc : rj;
}

// ---- the forward: one frame, each engine's steps -------------------------------------------------------------
struct Taps {
    const char* name = nullptr;
    float* out = nullptr;
    // "conv_pre" / "pre_tanh", or "ups_<i>" / "mrf_<i>" with stage i
    bool is(const char* tap, int i = -1) const {
        if (!name) return false;
        return i < 0 ? !strcmp(name, tap) : !strncmp(name, tap, 4) && atoi(name + 4) == i;
    }
};

// one micro-batch of a forward: utterances b0 .. b0 + nb - 1 on stream s
struct MicroBatch {
    int b0, nb;
    hipStream_t s;
    PassBufs buf;
    bool par;    // the MRF's ResBlocks as parallel chains
    float* wav;  // this micro-batch's waveform [nb][hop * T]
    bool tail;   // bf16: conv_post + tanh ride on the last pair launch (tail_fused_bf16)
    unsigned upfuse;  // bf16: bit i = ups_{i+1} rides on the pair launch that ends stage i (up_fused_bf16)
};

// tap copies: the engine's activation (bf16 channels-last or fp32 channel-major, its own layout) into the caller's fp32 tensor
int tap_copy(const vtts_hifigan* h, const MicroBatch& m, const void* src, float* dst, size_t n) {
    const hipError_t e = h->dtype == VTTS_BF16 ? launch_bf16_to_f32(src, dst, n, m.s)
                                               : hipMemcpyAsync(dst, src, n * sizeof(float), hipMemcpyDeviceToDevice, m.s);
    if (e != hipSuccess) return failf(VTTS_ERR_HIP, "tap copy failed: %s", hipGetErrorString(e));
    return VTTS_OK;
}

// x = (rb_0(x) + rb_1(x) [+ rb_2(x)]) / num_kernels with the ResBlocks' outputs in separate buffers (model.py:115-121): the same
// additions in the same order as the ACC_STORE / ACC_ADD / ACC_MEAN epilogues (device_common.h), hence the same bits.
__global__ __launch_bounds__(256) void mrf_mean_k(const float* __restrict__ y0, const float* __restrict__ y1, const float* __restrict__ y2,
                                                  float* __restrict__ out, size_t n, float div) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        float v = y0[i] + y1[i];
        if (y2) v = v + y2[i];
        out[i] = v / div;
    }
}

// fp32 / bf16x3 engine: channel-major fp32 activations [B][C][L]
float* f32(char* p) { return reinterpret_cast<float*>(p); }

int conv_pre_f32(vtts_hifigan* h, const MicroBatch& m, const float* mel, int T) {
    // conv_pre (model.py:110): mel [nb][T][num_mels] NWC -> S [nb][C0][T]
    const int nm = h->cfg.num_mels;
    return run_layer(h, h->layers[h->idx_pre], Act{mel, (long)T * nm, 1, nm}, m.nb, T, 1.0f, nullptr, f32(m.buf.S), ACC_STORE, 1.f, 0,
                     nullptr, m.s);
}

int upsample_f32(vtts_hifigan* h, const MicroBatch& m, int i, int L) {
    // x = ups_i(leaky_relu(x, 0.1))   (model.py:112-114)
    const Layer& up = h->layers[h->idx_ups[i]];
    return run_layer(h, up, Act{f32(m.buf.S), (long)up.cin * L, L, 1}, m.nb, L, 0.1f, nullptr, f32(m.buf.X), ACC_STORE, 1.f, 0, nullptr, m.s);
}

int mrf_f32(vtts_hifigan* h, const MicroBatch& m, int i, int L) {
    const int nk = h->cfg.num_kernels;
    const long CL = (long)h->layers[h->idx_ups[i]].cout * L;
    // one ResBlock of the MRF: X -> (T, C scratch) -> out with the given accumulate mode, on stream cs
    auto run_chain = [&](int j, float* out, int mode, float div, hipStream_t cs) -> int {
        const Layer* rb = &h->layers[h->idx_res[i * nk + j]];
        float* tT = f32(m.buf.T[j]);
        float* tC = f32(m.buf.C[j]);
        const float* cur = f32(m.buf.X);
        int rc;
        if (h->cfg.resblock == 2) {
            // ResBlock2: x = c_z(leaky_relu(x, 0.1)) + x, z = 0, 1 (model.py:69-74); the MRF sum / mean in the last epilogue
            if ((rc = run_layer(h, rb[0], Act{cur, CL, L, 1}, m.nb, L, 0.1f, cur, tC, ACC_STORE, 1.f, 0, nullptr, cs))) return rc;
            return run_layer(h, rb[1], Act{tC, CL, L, 1}, m.nb, L, 0.1f, tC, out, mode, div, 0, nullptr, cs);
        }
        const Route route = route_f32(h, rb, L);
        if (route == ROUTE_X3_RESBLOCK) return run_resblock_x3(h, rb, cur, m.nb, L, out, mode, div, cs);  // X -> out in one launch
        if (route == ROUTE_PAIRS || route == ROUTE_X3_PAIRS) {
            // fused pairs cannot run in place (a neighbour tile's halo would see updated columns): X -> T -> C -> out
            const bool x3 = route == ROUTE_X3_PAIRS;
            if ((rc = run_pair_f32(h, rb[0], rb[1], x3, cur, m.nb, L, tT, ACC_STORE, 1.f, cs))) return rc;
            if ((rc = run_pair_f32(h, rb[2], rb[3], x3, tT, m.nb, L, tC, ACC_STORE, 1.f, cs))) return rc;
            return run_pair_f32(h, rb[4], rb[5], x3, tC, m.nb, L, out, mode, div, cs);
        }
        for (int z = 0; z < 3; ++z) {
            // xt = c1(leaky_relu(x, 0.1))                       (model.py:46-47)
            if ((rc = run_layer(h, rb[2 * z], Act{cur, CL, L, 1}, m.nb, L, 0.1f, nullptr, tT, ACC_STORE, 1.f, 0, nullptr, cs))) return rc;
            // x = c2(leaky_relu(xt, 0.1)) + x                  (model.py:48-50); the last pair's output takes the MRF sum / mean (model.py:115-121)
            const bool last = z == 2;
            if ((rc = run_layer(h, rb[2 * z + 1], Act{tT, CL, L, 1}, m.nb, L, 0.1f, cur, last ? out : tC, last ? mode : ACC_STORE, last ? div : 1.f,
                                0, nullptr, cs)))
                return rc;
            cur = tC;
        }
        return VTTS_OK;
    };
    if (!m.par) {
        for (int j = 0; j < nk; ++j) {
            const int mode = (j == 0) ? ACC_STORE : (j == nk - 1 ? ACC_MEAN : ACC_ADD);
            if (int rc = run_chain(j, f32(m.buf.S), mode, (float)nk, m.s)) return rc;
        }
        return VTTS_OK;
    }
    // the ResBlocks side by side, each into its own buffers; ((y0 + y1) + y2) / nk afterwards: same additions, same order
    float* ys[3] = {f32(m.buf.Y[0]), f32(m.buf.Y[1]), f32(m.buf.Y[2])};
    if (int rc = run_chains_parallel(h, nk, m.s, [&](int j, hipStream_t cs) { return run_chain(j, ys[j], ACC_STORE, 1.f, cs); })) return rc;
    const size_t n = (size_t)m.nb * CL;
    hipLaunchKernelGGL(mrf_mean_k, dim3((unsigned)std::min<size_t>((n + 255) / 256, 4096)), dim3(256), 0, m.s, ys[0], ys[1], ys[2], f32(m.buf.S),
                       n, (float)nk);
    if (hipGetLastError() != hipSuccess) return failf(VTTS_ERR_HIP, "mrf_mean launch failed");
    return VTTS_OK;
}

int conv_post_f32(vtts_hifigan* h, const MicroBatch& m, int L, float* pre_act) {
    // tail: tanh(conv_post(leaky_relu(x)))  — slope 0.01, the jax default (model.py:122-124)
    const Layer& l = h->layers[h->idx_post];
    return run_layer(h, l, Act{f32(m.buf.S), (long)l.cin * L, L, 1}, m.nb, L, 0.01f, nullptr, m.wav, ACC_STORE, 1.f, 1, pre_act, m.s);
}

// bf16 engine.  Same dataflow as the fp32 one, with two differences that only bf16 needs:
//  * activations are channels-last bf16 [B][L][C] (a transposed convolution's [L][s*Cout] output IS the
//    [s*L][Cout] tensor);
//  * a tensor that is only ever consumed through LeakyReLU is stored already activated by its producer
//    (in fp32, before the bf16 rounding): conv_pre -> ups_0, xt = c1(.) -> c2, MRF mean -> next ups / conv_post.
//    Only the ResBlock's running x is stored raw (it is also the residual) and activated on load by c1.
int conv_pre_bf16(vtts_hifigan* h, const MicroBatch& m, const float* mel, int T) {
    const int nm = h->cfg.num_mels;
    return run_layer_bf16(h, h->layers[h->idx_pre], mel, nm, nm, m.nb, T, 1.0f, 0.1f, nullptr, m.buf.S, 0, 1.f, m.s);
}

int upsample_bf16(vtts_hifigan* h, const MicroBatch& m, int i, int L) {
    const Layer& up = h->layers[h->idx_ups[i]];
    return run_layer_bf16(h, up, m.buf.S, up.cin, up.cin, m.nb, L, 1.0f, 1.0f, nullptr, m.buf.X, 0, 1.f, m.s);
}

int mrf_bf16(vtts_hifigan* h, const MicroBatch& m, int i, int L) {
    const vtts_hifigan_cfg& c = h->cfg;
    const int nk = c.num_kernels;
    const int C = h->layers[h->idx_ups[i]].cout;
    const bool last_stage = i + 1 == c.num_upsamples;
    const float next_slope = last_stage ? 0.01f : 0.1f;  // model.py:112 / :122
    // one ResBlock of the MRF: X -> (tT, tC scratch) -> the shared accumulator S (store / accumulate / accumulate-and-divide in the
    // LAST kernel's epilogue); `before_last` runs right before that kernel is enqueued (the parallel schedule's ordering point)
    auto run_chain = [&](int j, hipStream_t cs, auto before_last) -> int {
        const Layer* rb = &h->layers[h->idx_res[i * nk + j]];
        char* tT = m.buf.T[j];
        char* tC = m.buf.C[j];
        const char* cur = m.buf.X;
        const bool last_rb = j == nk - 1;
        const float slope = last_rb ? next_slope : 1.0f;
        const int acc = j > 0 ? 1 : 0;
        const float div = last_rb ? (float)nk : 1.0f;
        int rc;
        if (c.resblock == 2) {
            // ResBlock2: x = c_z(leaky_relu(x, 0.1)) + x, z = 0, 1 (model.py:69-74): the running x is stored raw (it is the residual) and
            // activated on load; the MRF sum / mean and the consumer's LeakyReLU in the second convolution's epilogue.  X -> C -> S
            if ((rc = run_layer_bf16(h, rb[0], cur, C, C, m.nb, L, 0.1f, 1.0f, cur, tC, 0, 1.f, cs))) return rc;
            if ((rc = before_last())) return rc;
            return run_layer_bf16(h, rb[1], tC, C, C, m.nb, L, 0.1f, slope, tC, m.buf.S, acc, div, cs);
        }
        switch (route_bf16(h, rb)) {
            case ROUTE_RESBLOCK:  // the whole ResBlock in one kernel: X -> S
                if ((rc = before_last())) return rc;
                return run_resblock_bf16(h, rb, cur, m.nb, L, slope, m.buf.S, acc, div, cs);
            case ROUTE_PAIRS:
                // fused pairs cannot run in place (a neighbour tile's halo would see updated rows):
                // X -> T -> C -> S, with X kept for the other ResBlocks of the stage
                if ((rc = run_pair_bf16(h, rb[0], cur, m.nb, L, 1.0f, tT, 0, 1.f, cs))) return rc;
                if ((rc = run_pair_bf16(h, rb[2], tT, m.nb, L, 1.0f, tC, 0, 1.f, cs))) return rc;
                if ((rc = before_last())) return rc;
                // upfuse: z = ups_{i+1}(.) goes into X, which every chain's first pair has finished reading by now: this chain's ran earlier on this
                // stream, and in the parallel schedule before_last() has just made this launch wait for the previous chain's LAST kernel (and that one
                // for the chain before it), each of which follows its own chain's first pair in stream order
                if (last_rb && ((m.upfuse >> i) & 1))
                    return run_pair_bf16(h, rb[4], tC, m.nb, L, slope, m.buf.S, acc, div, cs, nullptr, &h->layers[h->idx_ups[i + 1]], m.buf.X);
                return run_pair_bf16(h, rb[4], tC, m.nb, L, slope, m.buf.S, acc, div, cs, last_stage && last_rb && m.tail ? m.wav : nullptr);
            default:
                for (int z = 0; z < 2; ++z) {
                    if ((rc = run_layer_bf16(h, rb[2 * z], cur, C, C, m.nb, L, 0.1f, 0.1f, nullptr, tT, 0, 1.f, cs))) return rc;
                    if ((rc = run_layer_bf16(h, rb[2 * z + 1], tT, C, C, m.nb, L, 1.0f, 1.0f, cur, tC, 0, 1.f, cs))) return rc;
                    cur = tC;
                }
                if ((rc = run_layer_bf16(h, rb[4], cur, C, C, m.nb, L, 0.1f, 0.1f, nullptr, tT, 0, 1.f, cs))) return rc;
                if ((rc = before_last())) return rc;
                return run_layer_bf16(h, rb[5], tT, C, C, m.nb, L, 1.0f, slope, cur, m.buf.S, acc, div, cs);
        }
    };
    if (!m.par) {
        for (int j = 0; j < nk; ++j)
            if (int rc = run_chain(j, m.s, [] { return VTTS_OK; })) return rc;
        return VTTS_OK;
    }
    // The ResBlocks side by side with scratch of their own.  Only a ResBlock's LAST kernel touches the shared accumulator (bf16, rounded
    // after every addition): those kernels are chained by events in the sequential order rb_0 -> rb_1 -> rb_2, so every sample sees the
    // same additions and roundings as one-after-the-other — the same bits.
    auto hip_rc = [&](hipError_t e, const char* what) -> int {
        return e == hipSuccess ? VTTS_OK : failf(VTTS_ERR_HIP, "%s failed: %s", what, hipGetErrorString(e));
    };
    return run_chains_parallel(h, nk, m.s, [&](int j, hipStream_t cs) -> int {
        int rc = run_chain(j, cs, [&]() -> int {
            return j > 0 ? hip_rc(hipStreamWaitEvent(cs, h->ev_chain[j - 1], 0), "hipStreamWaitEvent(chain)") : VTTS_OK;
        });
        if (!rc && j + 1 < nk) {
            if (!h->ev_chain[j]) rc = hip_rc(hipEventCreateWithFlags(&h->ev_chain[j], hipEventDisableTiming), "hipEventCreateWithFlags(chain)");
            if (!rc) rc = hip_rc(hipEventRecord(h->ev_chain[j], cs), "hipEventRecord(chain)");
        }
        return rc;
    });
}

int conv_post_bf16(vtts_hifigan* h, const MicroBatch& m, int L, float* pre_act) {
    const Layer& l = h->layers[h->idx_post];
    BConvArgs a;
    memset(&a, 0, sizeof(a));
    a.x = m.buf.S;
    a.wf = reinterpret_cast<const float*>(h->blob + l.off_w);
    a.bias = reinterpret_cast<const float*>(h->blob + l.off_b);
    a.B = m.nb;
    a.L = L;
    set_ragged(h, a, L);
    hipError_t e = launch_conv_post_bf16(a, m.wav, pre_act, m.s);
    if (e != hipSuccess) return failf(VTTS_ERR_HIP, "conv_post launch failed: %s", hipGetErrorString(e));
    return VTTS_OK;
}

// one engine's steps of a micro-batch; forward_impl runs them stage by stage
struct Engine {
    int (*conv_pre)(vtts_hifigan*, const MicroBatch&, const float* mel, int T);  // mel -> S
    int (*upsample)(vtts_hifigan*, const MicroBatch&, int i, int L);             // S -> X, L = stage i's input length
    int (*mrf)(vtts_hifigan*, const MicroBatch&, int i, int L);                  // X -> S, L = stage i's length
    int (*conv_post)(vtts_hifigan*, const MicroBatch&, int L, float* pre_act);   // S -> wav
};
constexpr Engine ENGINE_F32{conv_pre_f32, upsample_f32, mrf_f32, conv_post_f32};
constexpr Engine ENGINE_BF16{conv_pre_bf16, upsample_bf16, mrf_bf16, conv_post_bf16};

int run_micro_batch(vtts_hifigan* h, const Engine& e, const MicroBatch& m, const float* mel, int T, const Taps& tap) {
    const vtts_hifigan_cfg& c = h->cfg;
    const Layer& pre = h->layers[h->idx_pre];
    int rc;
    if ((rc = e.conv_pre(h, m, mel + (size_t)m.b0 * T * c.num_mels, T))) return rc;
    if (tap.is("conv_pre") && (rc = tap_copy(h, m, m.buf.S, tap.out + (size_t)m.b0 * pre.cout * T, (size_t)m.nb * pre.cout * T))) return rc;
    long L = T;
    for (int i = 0; i < c.num_upsamples; ++i) {
        const Layer& up = h->layers[h->idx_ups[i]];
        const bool up_done = i > 0 && ((m.upfuse >> (i - 1)) & 1);  // X already holds ups_i's output: it ran inside stage i - 1's last pair launch
        if (!up_done && (rc = e.upsample(h, m, i, (int)L))) return rc;
        L *= up.stride;
        const size_t CL = (size_t)up.cout * L;
        if (tap.is("ups_", i) && (rc = tap_copy(h, m, m.buf.X, tap.out + (size_t)m.b0 * CL, (size_t)m.nb * CL))) return rc;
        if ((rc = e.mrf(h, m, i, (int)L))) return rc;
        if (tap.is("mrf_", i) && (rc = tap_copy(h, m, m.buf.S, tap.out + (size_t)m.b0 * CL, (size_t)m.nb * CL))) return rc;
    }
    if (m.tail) return VTTS_OK;  // conv_post + tanh already ran inside the last pair launch
    return e.conv_post(h, m, (int)L, tap.is("pre_tanh") ? tap.out + (size_t)m.b0 * h->hop * T : nullptr);
}

int forward_impl(vtts_hifigan* h, const float* mel, int B, int T, float* wav, void* ws, size_t ws_bytes, hipStream_t s0,
                 const Taps& tap) {
    if (!h->blob) return failf(VTTS_ERR_STATE, "forward() before pack()/bind_packed()");
    if (B <= 0 || T <= 0) return failf(VTTS_ERR_INVALID, "B and T must be positive (got B=%d, T=%d)", B, T);
    if (int rc = check_pass_size(h, B, T)) return rc;
    const PassPlan p = plan_pass(h, B, T);
    if (ws_bytes < p.bytes() || !ws) return failf(VTTS_ERR_NOMEM, "workspace too small: %zu < %zu bytes", ws_bytes, p.bytes());
    if ((reinterpret_cast<uintptr_t>(ws) & 255) != 0) return failf(VTTS_ERR_INVALID, "workspace must be 256-B aligned");
    {
        hipError_t e = hipSetDevice(h->device);  // side streams / events are created lazily: on THIS handle's device
        if (e != hipSuccess) return failf(VTTS_ERR_HIP, "hipSetDevice(%d) failed: %s", h->device, hipGetErrorString(e));
    }
    const Engine& e = h->dtype == VTTS_BF16 ? ENGINE_BF16 : ENGINE_F32;
    const bool tail = h->dtype == VTTS_BF16 && !tap.name && tail_fused_bf16(h);
    unsigned upfuse = 0;
    for (int i = 1; h->dtype == VTTS_BF16 && i + 1 < h->cfg.num_upsamples; ++i)
        if (up_fused_bf16(h, i) && !tap.is("mrf_", i)) upfuse |= 1u << i;
    hipStream_t streams[4];
    int rc = fork_streams(h, p.nstr, s0, streams);
    for (int b0 = 0; b0 < B && !rc; b0 += p.mb) {
        const int si = (b0 / p.mb) % p.nstr;
        const MicroBatch m{b0, std::min(p.mb, B - b0), streams[si], p.buffers(ws, si, h->cfg.num_kernels), p.par, wav + (size_t)b0 * h->hop * T, tail, upfuse};
        h->cur_b0 = b0;
        rc = run_micro_batch(h, e, m, mel, T, tap);
    }
    // the only exit after the fork: a failed launch must not leave forked side streams un-joined
    const int rj = join_streams(h, p.nstr, s0);
    return rc ? rc : rj;
}

}  // namespace

// ================================ C ABI ==========================================================
VTTS_API int vtts_abi_version(void) { return VTTS_ABI_VERSION; }

VTTS_API const char* vtts_last_error(void) { return g_last_error.c_str(); }

VTTS_API int vtts_hifigan_create(const vtts_hifigan_cfg* cfg, int device, int dtype, vtts_hifigan** out) {
    if (!cfg || !out) return failf(VTTS_ERR_INVALID, "null argument");
    *out = nullptr;
    if (dtype != VTTS_F32 && dtype != VTTS_BF16 && dtype != VTTS_BF16X3) return failf(VTTS_ERR_INVALID, "unknown dtype %d", dtype);
    if (cfg->num_upsamples < 1 || cfg->num_upsamples > VTTS_MAX_UPSAMPLES)
        return failf(VTTS_ERR_INVALID, "num_upsamples %d out of range", cfg->num_upsamples);
    if (cfg->num_kernels < 1 || cfg->num_kernels > VTTS_MAX_KERNELS)
        return failf(VTTS_ERR_INVALID, "num_kernels %d out of range", cfg->num_kernels);
    if (cfg->num_mels < 1 || cfg->upsample_initial_channel < 1)
        return failf(VTTS_ERR_INVALID, "num_mels / upsample_initial_channel must be positive");
    if (cfg->upsample_initial_channel % (1 << cfg->num_upsamples) != 0)
        return failf(VTTS_ERR_INVALID, "upsample_initial_channel %d not divisible by 2^%d", cfg->upsample_initial_channel,
                     cfg->num_upsamples);
    for (int i = 0; i < cfg->num_upsamples; ++i)
        if (cfg->upsample_rates[i] < 1 || cfg->upsample_kernel_sizes[i] < cfg->upsample_rates[i])
            return failf(VTTS_ERR_INVALID, "bad upsample stage %d (rate %d, kernel %d)", i, cfg->upsample_rates[i],
                         cfg->upsample_kernel_sizes[i]);
    for (int j = 0; j < cfg->num_kernels; ++j) {
        if (cfg->resblock_kernel_sizes[j] < 1 || cfg->resblock_kernel_sizes[j] % 2 == 0)
            return failf(VTTS_ERR_INVALID, "resblock kernel size %d must be odd", cfg->resblock_kernel_sizes[j]);
        for (int z = 0; z < (cfg->resblock == 2 ? 2 : 3); ++z)
            if (cfg->resblock_dilation_sizes[j][z] < 1) return failf(VTTS_ERR_INVALID, "dilation must be >= 1");
    }
    if (cfg->resblock != 0 && cfg->resblock != 1 && cfg->resblock != 2)
        return failf(VTTS_ERR_INVALID, "resblock must be 1 (ResBlock1) or 2 (ResBlock2), got %d", cfg->resblock);
    if (device < 0) return failf(VTTS_ERR_INVALID, "device %d out of range", device);
    // the device itself is first touched in pack()/bind_packed(): planning needs no GPU
    auto* h = new (std::nothrow) vtts_hifigan();
    if (!h) return failf(VTTS_ERR_NOMEM, "host allocation failed");
    h->cfg = *cfg;
    if (h->cfg.resblock == 0) h->cfg.resblock = 1;
    h->device = device;
    h->dtype = dtype == VTTS_BF16X3 ? VTTS_F32 : dtype;
    h->x3 = dtype == VTTS_BF16X3;
    const int rc = build_layers(h);
    if (rc != VTTS_OK) {
        delete h;
        return rc;
    }
    *out = h;
    return VTTS_OK;
}

static void drop_graphs(vtts_hifigan* h) {
    for (auto& g : h->graphs) {
        if (g.exec) (void)hipGraphExecDestroy(g.exec);
        if (g.graph) (void)hipGraphDestroy(g.graph);
    }
    h->graphs.clear();
    if (h->cap_stream) (void)hipStreamDestroy(h->cap_stream);
    h->cap_stream = nullptr;
}

VTTS_API void vtts_hifigan_destroy(vtts_hifigan* h) {
    if (!h) return;
    for (int i = 0; i < 3; ++i) {
        if (h->side_streams[i]) (void)hipStreamDestroy(h->side_streams[i]);
        if (h->ev_join[i]) (void)hipEventDestroy(h->ev_join[i]);
    }
    if (h->ev_fork) (void)hipEventDestroy(h->ev_fork);
    for (hipEvent_t e : h->ev_chain)
        if (e) (void)hipEventDestroy(e);
    drop_graphs(h);
    for (auto& p : h->prof_events) {
        (void)hipEventDestroy(p.first);
        (void)hipEventDestroy(p.second);
    }
    delete h;
}

VTTS_API int vtts_hifigan_num_params(const vtts_hifigan* h, int* n) {
    if (!h || !n) return failf(VTTS_ERR_INVALID, "null argument");
    *n = 2 * (int)h->layers.size();
    return VTTS_OK;
}

VTTS_API int vtts_hifigan_param_info(const vtts_hifigan* h, int i, const char** key, const char** which, int64_t shape[3],
                                     int* ndim) {
    if (!h || !key || !which || !shape || !ndim) return failf(VTTS_ERR_INVALID, "null argument");
    if (i < 0 || i >= 2 * (int)h->layers.size()) return failf(VTTS_ERR_INVALID, "parameter index %d out of range", i);
    const Layer& l = h->layers[i / 2];
    *key = l.key.c_str();
    if (i % 2 == 0) {
        *which = "w";
        *ndim = 3;
        shape[0] = l.k;
        shape[1] = (l.kind == KIND_CONV) ? l.cin : l.cout;
        shape[2] = (l.kind == KIND_CONV) ? l.cout : l.cin;
    } else {
        *which = "b";
        *ndim = 1;
        shape[0] = l.cout;
        shape[1] = shape[2] = 0;
    }
    return VTTS_OK;
}

VTTS_API int vtts_hifigan_set_param(vtts_hifigan* h, const char* key, const char* which, const float* host,
                                    const int64_t* shape, int ndim) {
    if (!h || !key || !which || !host || !shape) return failf(VTTS_ERR_INVALID, "null argument");
    Layer* l = find_layer(h, key);
    if (!l) return failf(VTTS_ERR_INVALID, "unknown parameter module '%s'", key);
    if (!strcmp(which, "w")) {
        const int64_t d1 = (l->kind == KIND_CONV) ? l->cin : l->cout;
        const int64_t d2 = (l->kind == KIND_CONV) ? l->cout : l->cin;
        if (ndim != 3 || shape[0] != l->k || shape[1] != d1 || shape[2] != d2)
            return failf(VTTS_ERR_SHAPE, "%s/w: expected [%d,%lld,%lld]", key, l->k, (long long)d1, (long long)d2);
        l->w.assign(host, host + (size_t)l->k * l->cin * l->cout);
        l->have_w = true;
    } else if (!strcmp(which, "b")) {
        if (ndim != 1 || shape[0] != l->cout) return failf(VTTS_ERR_SHAPE, "%s/b: expected [%d]", key, l->cout);
        l->b.assign(host, host + l->cout);
        l->have_b = true;
    } else {
        return failf(VTTS_ERR_INVALID, "parameter name must be \"w\" or \"b\", got \"%s\"", which);
    }
    return VTTS_OK;
}

VTTS_API int vtts_hifigan_packed_bytes(const vtts_hifigan* h, size_t* bytes) {
    if (!h || !bytes) return failf(VTTS_ERR_INVALID, "null argument");
    *bytes = h->blob_bytes;
    return VTTS_OK;
}

VTTS_API int vtts_hifigan_pack(vtts_hifigan* h, void* dev_blob, size_t blob_bytes, vtts_stream stream) {
    if (!h) return failf(VTTS_ERR_INVALID, "null argument");
    if (int rc = check_blob(dev_blob, blob_bytes, h->blob_bytes)) return rc;
    for (auto& l : h->layers)
        if (!l.have_w || !l.have_b) return failf(VTTS_ERR_MISSING, "parameter %s/%s was never set", l.key.c_str(), l.have_w ? "b" : "w");
    std::vector<char> host(h->blob_bytes, 0);
    if (h->dtype == VTTS_BF16) {
        for (auto& l : h->layers) {
            float* bb = reinterpret_cast<float*>(host.data() + l.off_b);
            for (int i = 0; i < l.coutp; ++i) bb[i] = l.b[i % l.cout];  // transposed conv rows are (phase, co)
            if (l.bcls < BCLS_NONE) {  // conv_post keeps plain fp32 weights
                memcpy(host.data() + l.off_w, l.w.data(), l.w.size() * sizeof(float));
                continue;
            }
            const BPackGeom g = bf16_pack_geom(l.bcls, l.kind == KIND_CONVT ? 3 : l.k);
            if (l.kind == KIND_CONVT) {
                // ConvTranspose1d(k = 2s) == Conv1d(Cin -> s*Cout, k = 3, pad 1) on channels-last data:
                // phase r (group g = r / (s/2)) reads frames q + g - 1 + m (m = 0,1) through tap
                // j = s*(g - 1 + m) + pad_a - r; the third frame of each phase gets zero weights.
                const int sdt = l.stride, coutp = l.coutp;
                std::vector<float> wc((size_t)3 * l.cin * coutp, 0.f);
                for (int r = 0; r < sdt; ++r) {
                    const int gq = r / (sdt / 2);
                    for (int m = 0; m < 2; ++m) {
                        const int f = gq + m, j = sdt * (gq - 1 + m) + l.pad_a - r;
                        for (int co = 0; co < l.cout; ++co)
                            for (int ci = 0; ci < l.cin; ++ci)
                                wc[((size_t)f * l.cin + ci) * coutp + r * l.cout + co] = l.w[((size_t)j * l.cout + co) * l.cin + ci];
                    }
                }
                bf16_pack(wc.data(), l.cin, g, reinterpret_cast<unsigned short*>(host.data() + l.off_wb));
                if (l.has_ug) bf16_pack(wc.data(), l.cin, convt_g_pack_geom(l.bcls), reinterpret_cast<unsigned short*>(host.data() + l.off_ug));
            } else {
                bf16_pack(l.w.data(), l.cin, g, reinterpret_cast<unsigned short*>(host.data() + l.off_wb));
                if (l.has_ug) bf16_pack(l.w.data(), l.cin, convt_g_pack_geom(l.bcls), reinterpret_cast<unsigned short*>(host.data() + l.off_ug));  // conv_pre
            }
        }
        for (size_t i = 0; i + 1 < h->layers.size(); ++i) {
            const Layer& c1 = h->layers[i];
            if (!c1.has_pair) continue;
            const Layer& c2 = h->layers[i + 1];
            const BPackGeom pg = pair_g_pack_geom(c1.cin, c1.k);
            const size_t half = bf16_packed_bytes(pg);
            pair_g_pack(c1.w.data(), c1.cin, c1.k, reinterpret_cast<unsigned short*>(host.data() + c1.off_pw));  // in its class's fragment order
            pair_g_pack(c2.w.data(), c2.cin, c1.k, reinterpret_cast<unsigned short*>(host.data() + c1.off_pw + half));
            float* pb = reinterpret_cast<float*>(host.data() + c1.off_pb);
            memcpy(pb, c1.b.data(), c1.cin * sizeof(float));
            memcpy(pb + c1.cin, c2.b.data(), c1.cin * sizeof(float));
        }
        for (size_t i = 0; i + 5 < h->layers.size(); ++i) {
            const Layer& c0 = h->layers[i];
            if (!c0.has_rb) continue;
            const BPackGeom pg = pair_g_pack_geom(c0.cin, c0.k);
            const size_t one = bf16_packed_bytes(pg);
            float* rb = reinterpret_cast<float*>(host.data() + c0.off_rb);
            for (int q = 0; q < 6; ++q) {
                const Layer& l = h->layers[i + q];
                bf16_pack(l.w.data(), l.cin, pg, reinterpret_cast<unsigned short*>(host.data() + c0.off_rw + q * one));
                memcpy(rb + (size_t)q * c0.cin, l.b.data(), c0.cin * sizeof(float));
            }
        }
    }
    for (auto& l : h->layers) {
        if (h->dtype == VTTS_BF16) break;
        memcpy(host.data() + l.off_w, l.w.data(), l.w.size() * sizeof(float));
        memcpy(host.data() + l.off_b, l.b.data(), l.b.size() * sizeof(float));
        if (l.has_x3 && &l == &h->layers[h->idx_pre]) conv_pre_x3_pack(l.w.data(), reinterpret_cast<unsigned short*>(host.data() + l.off_x3));
        else if (l.has_x3 && l.kind == KIND_CONVT) convt_x3_pack(l.w.data(), l.cin, l.cout, l.k, l.stride, l.pad_a, reinterpret_cast<unsigned short*>(host.data() + l.off_x3));
        else if (l.has_x3) pair_x3_pack(l.w.data(), l.cin, l.k, reinterpret_cast<unsigned short*>(host.data() + l.off_x3));
        if (l.has_wp && l.kind == KIND_CONV)
            conv1d_f32_mfma_pack(l.w.data(), l.cin, l.cout, l.k, reinterpret_cast<float*>(host.data() + l.off_wp));
        else if (l.has_wp)
            convT1d_f32_mfma_pack(l.w.data(), l.cin, l.cout, l.k, l.stride, l.pad_a, reinterpret_cast<float*>(host.data() + l.off_wp));
    }
    HIP_TRY(hipSetDevice(h->device));
    if (int rc = upload_blob(dev_blob, host.data(), h->blob_bytes, static_cast<hipStream_t>(stream), "the generator's weights")) return rc;
    h->blob = static_cast<char*>(dev_blob);
    ++h->epoch;  // captured graphs hold the old blob's addresses
    return VTTS_OK;
}

VTTS_API int vtts_hifigan_bind_packed(vtts_hifigan* h, void* dev_blob, size_t blob_bytes) {
    if (!h) return failf(VTTS_ERR_INVALID, "null argument");
    if (int rc = check_blob(dev_blob, blob_bytes, h->blob_bytes)) return rc;
    h->blob = static_cast<char*>(dev_blob);
    ++h->epoch;  // captured graphs hold the old blob's addresses
    return VTTS_OK;
}

VTTS_API int vtts_hifigan_workspace_bytes(const vtts_hifigan* h, int B, int T, size_t* bytes) {
    if (!h || !bytes) return failf(VTTS_ERR_INVALID, "null argument");
    if (B <= 0 || T <= 0) return failf(VTTS_ERR_INVALID, "B and T must be positive");
    if (int rc = check_pass_size(h, B, T)) return rc;
    *bytes = plan_pass(h, B, T).bytes();
    return VTTS_OK;
}

// Small launches are a chain of ~40 short kernels over up to three streams; replaying them as ONE hipGraph removes the host's
// launch / event calls and the cross-stream waits from the critical path (bf16, one 512-frame utterance: 0.81 -> 0.70 ms).  A graph
// bakes in every pointer, so it is keyed by (mel, wav, workspace, B, T) and by an epoch that options and the weight blob bump; it is
// captured the GRAPH_AFTER-th time the same key shows up (the eager runs before it also finish every lazy initialisation: side
// streams, events, function attributes), replayed afterwards, and anything unexpected falls back to the eager path.
constexpr int GRAPH_SLOTS = 8;
constexpr int GRAPH_AFTER = 8;  // capture + instantiate cost about a millisecond, once: only a key that keeps coming back pays it
int forward_maybe_graphed(vtts_hifigan* h, const float* mel, int B, int T, float* wav, void* ws, size_t ws_bytes, hipStream_t s) {
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    if (!h->opt_graph || h->opt_profile || B <= 0 || T <= 0 || !h->blob || !plan_pass(h, B, T).par ||
        hipStreamIsCapturing(s, &st) != hipSuccess || st != hipStreamCaptureStatusNone)  // inside the CALLER's capture: just enqueue
        return forward_impl(h, mel, B, T, wav, ws, ws_bytes, s, Taps{});
    if (hipSetDevice(h->device) != hipSuccess) return failf(VTTS_ERR_HIP, "hipSetDevice(%d) failed", h->device);  // graph launches too run on THIS handle's device
    vtts_hifigan::GraphEntry* e = nullptr;
    for (auto& g : h->graphs)
        if (g.mel == mel && g.wav == wav && g.ws == ws && g.B == B && g.T == T) e = &g;
    if (e && e->epoch != h->epoch) {  // stale: start over
        if (e->exec) (void)hipGraphExecDestroy(e->exec);
        if (e->graph) (void)hipGraphDestroy(e->graph);
        e->exec = nullptr;
        e->graph = nullptr;
        e->seen = 0;
        e->epoch = h->epoch;
    }
    if (!e) {
        if ((int)h->graphs.size() < GRAPH_SLOTS) {
            h->graphs.emplace_back();
            e = &h->graphs.back();
        } else {
            e = &h->graphs[0];
            for (auto& g : h->graphs)
                if (g.last_use < e->last_use) e = &g;
            if (e->exec) (void)hipGraphExecDestroy(e->exec);
            if (e->graph) (void)hipGraphDestroy(e->graph);
        }
        *e = vtts_hifigan::GraphEntry{};
        e->mel = mel; e->wav = wav; e->ws = ws; e->B = B; e->T = T; e->epoch = h->epoch;
    }
    e->last_use = ++h->use_clock;
    if (e->exec) {
        hipError_t le = hipGraphLaunch(e->exec, s);
        if (le == hipSuccess) return VTTS_OK;
        (void)hipGetLastError();
        e->seen = -1;  // never again for this key
        (void)hipGraphExecDestroy(e->exec);
        e->exec = nullptr;
        return forward_impl(h, mel, B, T, wav, ws, ws_bytes, s, Taps{});
    }
    if (e->seen < 0 || ++e->seen < GRAPH_AFTER) return forward_impl(h, mel, B, T, wav, ws, ws_bytes, s, Taps{});
    // a key that keeps coming back: record this call's launches into a graph (on a stream of the handle's own: the caller's may be the legacy
    // default stream, which cannot be captured), then launch the graph on the caller's stream
    if (!h->cap_stream && hipStreamCreateWithFlags(&h->cap_stream, hipStreamNonBlocking) != hipSuccess) {
        (void)hipGetLastError();
        h->cap_stream = nullptr;
        e->seen = -1;
        return forward_impl(h, mel, B, T, wav, ws, ws_bytes, s, Taps{});
    }
    if (hipStreamBeginCapture(h->cap_stream, hipStreamCaptureModeThreadLocal) != hipSuccess) {
        (void)hipGetLastError();
        e->seen = -1;
        return forward_impl(h, mel, B, T, wav, ws, ws_bytes, s, Taps{});
    }
    const int rc = forward_impl(h, mel, B, T, wav, ws, ws_bytes, h->cap_stream, Taps{});
    hipGraph_t g = nullptr;
    hipError_t ce = hipStreamEndCapture(h->cap_stream, &g);
    hipGraphExec_t ex = nullptr;
    if (rc == VTTS_OK && ce == hipSuccess && g && hipGraphInstantiate(&ex, g, nullptr, nullptr, 0) == hipSuccess && hipGraphLaunch(ex, s) == hipSuccess) {
        e->graph = g;
        e->exec = ex;
        return VTTS_OK;
    }
    (void)hipGetLastError();
    if (ex) (void)hipGraphExecDestroy(ex);
    if (g) (void)hipGraphDestroy(g);
    e->seen = -1;
    if (rc) return rc;  // the enqueue itself failed: report that
    return forward_impl(h, mel, B, T, wav, ws, ws_bytes, s, Taps{});  // nothing ran during the capture: run it now
}

VTTS_API int vtts_hifigan_forward(vtts_hifigan* h, const float* mel_dev, int B, int T, float* wav_dev, void* workspace,
                                  size_t workspace_bytes, vtts_stream stream) {
    if (!h || !mel_dev || !wav_dev) return failf(VTTS_ERR_INVALID, "null argument");
    return forward_maybe_graphed(h, mel_dev, B, T, wav_dev, workspace, workspace_bytes, static_cast<hipStream_t>(stream));
}

VTTS_API int vtts_hifigan_forward_ragged(vtts_hifigan* h, const float* mel_dev, const int32_t* frames_dev, int B, int T, float* wav_dev,
                                         void* workspace, size_t workspace_bytes, vtts_stream stream) {
    if (!h || !mel_dev || !frames_dev || !wav_dev) return failf(VTTS_ERR_INVALID, "null argument");
    if (B <= 0 || T <= 0) return failf(VTTS_ERR_INVALID, "B and T must be positive (got B=%d, T=%d)", B, T);
    hipStream_t s = static_cast<hipStream_t>(stream);
    HIP_TRY(hipMemsetAsync(wav_dev, 0, (size_t)B * h->hop * T * sizeof(float), s));  // samples past an utterance's end
    h->cur_lens = frames_dev;
    h->cur_T = T;
    const int rc = forward_impl(h, mel_dev, B, T, wav_dev, workspace, workspace_bytes, s, Taps{});
    h->cur_lens = nullptr;
    h->cur_T = 0;
    return rc;
}

VTTS_API int vtts_hifigan_tap_elems(const vtts_hifigan* h, const char* tap, int B, int T, size_t* elems) {
    if (!h || !tap || !elems) return failf(VTTS_ERR_INVALID, "null argument");
    const vtts_hifigan_cfg& c = h->cfg;
    if (!strcmp(tap, "pre_tanh")) {
        *elems = (size_t)B * h->hop * T;
        return VTTS_OK;
    }
    if (!strcmp(tap, "conv_pre")) {
        *elems = (size_t)B * c.upsample_initial_channel * T;
        return VTTS_OK;
    }
    if (!strncmp(tap, "ups_", 4) || !strncmp(tap, "mrf_", 4)) {
        const int i = atoi(tap + 4);
        if (i < 0 || i >= c.num_upsamples) return failf(VTTS_ERR_INVALID, "tap stage %d out of range", i);
        long L = T;
        for (int q = 0; q <= i; ++q) L *= c.upsample_rates[q];
        *elems = (size_t)B * (c.upsample_initial_channel >> (i + 1)) * L;
        return VTTS_OK;
    }
    return failf(VTTS_ERR_INVALID, "unknown tap '%s'", tap);
}

VTTS_API int vtts_hifigan_forward_tap(vtts_hifigan* h, const float* mel_dev, int B, int T, float* wav_dev, void* workspace,
                                      size_t workspace_bytes, vtts_stream stream, const char* tap, float* tap_dev) {
    if (!h || !mel_dev || !wav_dev || !tap || !tap_dev) return failf(VTTS_ERR_INVALID, "null argument");
    size_t n = 0;
    int rc = vtts_hifigan_tap_elems(h, tap, B, T, &n);
    if (rc) return rc;
    Taps t;
    t.name = tap;
    t.out = tap_dev;
    return forward_impl(h, mel_dev, B, T, wav_dev, workspace, workspace_bytes, static_cast<hipStream_t>(stream), t);
}

// device scratch of the test hooks below: released on every return path
struct DevBuf {
    void* p = nullptr;
    ~DevBuf() {
        if (p) (void)hipFree(p);
    }
};

VTTS_API int vtts_hifigan_run_module(vtts_hifigan* h, const char* key, const float* x_dev, int B, int L, float slope_in,
                                     const float* res_dev, float* y_dev, vtts_stream stream) {
    if (!h || !key || !x_dev || !y_dev) return failf(VTTS_ERR_INVALID, "null argument");
    if (!h->blob) return failf(VTTS_ERR_STATE, "run_module() before pack()/bind_packed()");
    if (B <= 0 || L <= 0) return failf(VTTS_ERR_INVALID, "B and L must be positive");
    Layer* l = find_layer(h, key);
    if (!l) return failf(VTTS_ERR_INVALID, "unknown module '%s'", key);
    const bool is_pre = (l == &h->layers[h->idx_pre]);
    const bool is_post = (l == &h->layers[h->idx_post]);
    if (h->dtype == VTTS_BF16) {
        // the bf16 kernels form LeakyReLU as max(v, slope * v) (bf16_common.h: lrelu_f), valid for slopes in (0, 1]: the model's are 0.1 and 0.01
        if (!(slope_in > 0.0f && slope_in <= 1.0f)) return failf(VTTS_ERR_INVALID, "run_module(): slope_in must lie in (0, 1] on a bf16 handle (got %g)", slope_in);
        // test hook: fp32 channels-last in/out, converted through temporary bf16 buffers
        hipStream_t st = static_cast<hipStream_t>(stream);
        const size_t nx = (size_t)B * L * l->cin, ny = (size_t)B * L * (l->kind == KIND_CONVT ? l->stride : 1) * l->cout;
        DevBuf xbuf, rbuf, ybuf;  // freed on every path (hipFree waits for the device)
        void *&xb = xbuf.p, *&rb = rbuf.p, *&yb = ybuf.p;
        int rc = VTTS_OK;
        if (is_post) {
            HIP_TRY(hipMalloc(&xb, nx * 2));
            if (launch_f32_to_bf16(x_dev, xb, nx, st) != hipSuccess) rc = failf(VTTS_ERR_HIP, "conversion launch failed");
            BConvArgs a;
            memset(&a, 0, sizeof(a));
            a.x = xb;
            a.wf = reinterpret_cast<const float*>(h->blob + l->off_w);
            a.bias = reinterpret_cast<const float*>(h->blob + l->off_b);
            a.B = B;
            a.L = L;
            if (!rc && launch_conv_post_bf16(a, y_dev, nullptr, st) != hipSuccess) rc = failf(VTTS_ERR_HIP, "conv_post launch failed");
        } else {
            HIP_TRY(hipMalloc(&yb, ny * 2));
            if (!is_pre) {
                HIP_TRY(hipMalloc(&xb, nx * 2));
                if (launch_f32_to_bf16(x_dev, xb, nx, st) != hipSuccess) rc = failf(VTTS_ERR_HIP, "conversion launch failed");
            }
            if (res_dev) {
                HIP_TRY(hipMalloc(&rb, ny * 2));
                if (launch_f32_to_bf16(res_dev, rb, ny, st) != hipSuccess) rc = failf(VTTS_ERR_HIP, "conversion launch failed");
            }
            if (!rc) rc = run_layer_bf16(h, *l, is_pre ? static_cast<const void*>(x_dev) : xb, l->cin, l->cin, B, L, slope_in, 1.0f, rb, yb, 0, 1.f, st);
            if (!rc && launch_bf16_to_f32(yb, y_dev, ny, st) != hipSuccess) rc = failf(VTTS_ERR_HIP, "conversion launch failed");
        }
        hipError_t e = hipStreamSynchronize(st);
        if (!rc && e != hipSuccess) rc = failf(VTTS_ERR_HIP, "run_module failed: %s", hipGetErrorString(e));
        return rc;
    }
    Act x = is_pre ? Act{x_dev, (long)L * l->cin, 1, l->cin} : Act{x_dev, (long)l->cin * L, L, 1};
    return run_layer(h, *l, x, B, L, slope_in, res_dev, y_dev, ACC_STORE, 1.f, is_post ? 1 : 0, nullptr,
                     static_cast<hipStream_t>(stream));
}

VTTS_API int vtts_hifigan_run_pair(vtts_hifigan* h, const char* key_c1, const float* x_dev, int B, int L, float* y_dev, vtts_stream stream) {
    if (!h || !key_c1 || !x_dev || !y_dev) return failf(VTTS_ERR_INVALID, "null argument");
    if (!h->blob) return failf(VTTS_ERR_STATE, "run_pair() before pack()/bind_packed()");
    if (B <= 0 || L <= 0) return failf(VTTS_ERR_INVALID, "B and L must be positive");
    Layer* l = find_layer(h, key_c1);
    const Layer* c2 = l && l + 1 < h->layers.data() + h->layers.size() ? l + 1 : nullptr;
    if (h->dtype == VTTS_F32) {
        // fp32 / bf16x3 handle: x_dev / y_dev are [B, C, L] channel-major (the fp32 engine's layout); asynchronous on `stream`
        const bool x3 = c2 && pair_x3_wanted(h, *l, *c2, L);
        if (!x3 && (!c2 || !pair_f32_fusable(*l, *c2, L)))
            return failf(VTTS_ERR_INVALID, "'%s' is not the first convolution of a ResBlock pair the fused fp32 kernel covers (C in {32, 64, 128}, L a multiple of 4)", key_c1);
        return run_pair_f32(h, *l, *c2, x3, x_dev, B, L, y_dev, ACC_STORE, 1.f, static_cast<hipStream_t>(stream));
    }
    if (!l || !l->has_pair) return failf(VTTS_ERR_INVALID, "'%s' is not the first convolution of a fused ResBlock pair", key_c1);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const size_t n = (size_t)B * L * l->cin;
    DevBuf xbuf, ybuf;
    void *&xb = xbuf.p, *&yb = ybuf.p;
    HIP_TRY(hipMalloc(&xb, n * 2));
    HIP_TRY(hipMalloc(&yb, n * 2));
    int rc = VTTS_OK;
    if (launch_f32_to_bf16(x_dev, xb, n, st) != hipSuccess) rc = failf(VTTS_ERR_HIP, "conversion launch failed");
    if (!rc) rc = run_pair_bf16(h, *l, xb, B, L, 1.0f, yb, 0, 1.f, st);
    if (!rc && launch_bf16_to_f32(yb, y_dev, n, st) != hipSuccess) rc = failf(VTTS_ERR_HIP, "conversion launch failed");
    hipError_t e = hipStreamSynchronize(st);
    if (!rc && e != hipSuccess) rc = failf(VTTS_ERR_HIP, "run_pair failed: %s", hipGetErrorString(e));
    return rc;
}

// the ragged state of a test hook's launches (set_ragged reads it): rows_dev as a.lens with len_mul = 1; cleared on every return path
struct RowsScope {
    vtts_hifigan* h;
    RowsScope(vtts_hifigan* h_, const int32_t* rows_dev, int L) : h(h_) {
        h->cur_lens = rows_dev;
        h->cur_T = rows_dev ? L : 0;
        h->cur_b0 = 0;
    }
    ~RowsScope() {
        h->cur_lens = nullptr;
        h->cur_T = 0;
        h->cur_b0 = 0;
    }
};

VTTS_API int vtts_hifigan_run_resblock(vtts_hifigan* h, const char* key_c1_0, int route, const float* x_dev, const int32_t* rows_dev, int B, int L,
                                       float slope_out, int acc_add, float div, float* y_dev, vtts_stream stream) {
    if (!h || !key_c1_0 || !x_dev || !y_dev) return failf(VTTS_ERR_INVALID, "null argument");
    if (!h->blob) return failf(VTTS_ERR_STATE, "run_resblock() before pack()/bind_packed()");
    if (B <= 0 || L <= 0) return failf(VTTS_ERR_INVALID, "B and L must be positive");
    if (B > 65535) return failf(VTTS_ERR_INVALID, "at most 65535 utterances per launch (got %d)", B);
    if (route != 0 && route != 1 && !(route == 2 && h->dtype == VTTS_F32))
        return failf(VTTS_ERR_INVALID, "route must be 0 (the whole-ResBlock kernel), 1 (three pair launches) or, on an fp32 / bf16x3 handle, 2 (six convolution launches), got %d", route);
    if ((acc_add != 0 && acc_add != 1) || !(div > 0.0f) || !std::isfinite(div))
        return failf(VTTS_ERR_INVALID, "run_resblock(): acc_add must be 0 or 1 and div a positive number (got %d, %g)", acc_add, div);
    const Layer* rb = nullptr;  // rb[0..5] = c1_0, c2_0, c1_1, c2_1, c1_2, c2_2
    for (size_t r = 0; r < h->idx_res.size() && h->cfg.resblock != 2; ++r)
        if (h->layers[h->idx_res[r]].key == key_c1_0) rb = &h->layers[h->idx_res[r]];
    if (!rb) return failf(VTTS_ERR_INVALID, "'%s' is not the first convolution (convs1_0) of a ResBlock1", key_c1_0);
    const int C = rb[0].cin;
    if ((size_t)L * C * elem_bytes(h) >= ((size_t)1 << 31))
        return failf(VTTS_ERR_INVALID, "L=%d rows of %d channels are too long for one launch (limit 2^31 bytes per utterance)", L, C);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const size_t n = (size_t)B * L * C;
    RowsScope rows(h, rows_dev, L);
    if (h->dtype == VTTS_F32) {
        // fp32 / bf16x3 handle: x_dev / y_dev are [B, C, L] channel-major, y_dev is the launch's own in-out tensor.  These engines' epilogues
        // have no output activation (the consumer applies it on load)
        if (slope_out != 1.0f) return failf(VTTS_ERR_INVALID, "run_resblock(): slope_out must be 1 on an fp32 / bf16x3 handle (got %g)", slope_out);
        if (!acc_add && div != 1.0f) return failf(VTTS_ERR_INVALID, "run_resblock(): div without acc_add is not an accumulate mode of the fp32 engine");
        const int mode = !acc_add ? ACC_STORE : (div != 1.0f ? ACC_MEAN : ACC_ADD);
        if (route == 0) {
            if (!resblock_x3_runnable(h, rb, L))
                return failf(VTTS_ERR_INVALID, "'%s': no whole-ResBlock kernel for this ResBlock on this handle (bf16x3, C = 32 / 64 / 128)", key_c1_0);
            return run_resblock_x3(h, rb, x_dev, B, L, y_dev, mode, div, st);
        }
        if (route == 2) {
            // the six convolutions one by one, as mrf_f32's ROUTE_CONVS branch: c1 -> T; c2 (+ cur) -> C, the last one -> y_dev with the mode
            DevBuf tbuf, cbuf;
            HIP_TRY(hipMalloc(&tbuf.p, n * sizeof(float)));
            HIP_TRY(hipMalloc(&cbuf.p, n * sizeof(float)));
            float *tT = static_cast<float*>(tbuf.p), *tC = static_cast<float*>(cbuf.p);
            const long CL = (long)C * L;
            const float* cur = x_dev;
            for (int z = 0; z < 3; ++z) {
                int rc;
                if ((rc = run_layer(h, rb[2 * z], Act{cur, CL, L, 1}, B, L, 0.1f, nullptr, tT, ACC_STORE, 1.f, 0, nullptr, st))) return rc;
                const bool last = z == 2;
                if ((rc = run_layer(h, rb[2 * z + 1], Act{tT, CL, L, 1}, B, L, 0.1f, cur, last ? y_dev : tC, last ? mode : ACC_STORE, last ? div : 1.f,
                                    0, nullptr, st)))
                    return rc;
                cur = tC;
            }
            return VTTS_OK;
        }
        bool x3 = h->x3 && h->opt_kernels == 0, fp = h->opt_kernels == 0;  // the split-operand pair kernel, else the fp32 one, as route_f32 picks them
        for (int z = 0; z < 3; ++z) {
            const Layer &c1 = rb[2 * z], &c2 = rb[2 * z + 1];
            x3 = x3 && c1.has_x3 && c2.has_x3 && c2.k == c1.k && c2.dil == 1 && c2.cin == c1.cin && pair_x3_supported(c1.cin, c1.k, c1.dil, L);
            fp = fp && pair_f32_fusable(c1, c2, L);
        }
        if (!x3 && !fp) return failf(VTTS_ERR_INVALID, "'%s': the fused pair kernels do not cover this ResBlock at L=%d", key_c1_0, L);
        DevBuf tbuf, cbuf;  // X -> T -> C -> y, as mrf_f32; released (hipFree waits for the device) on every path
        HIP_TRY(hipMalloc(&tbuf.p, n * sizeof(float)));
        HIP_TRY(hipMalloc(&cbuf.p, n * sizeof(float)));
        float *tT = static_cast<float*>(tbuf.p), *tC = static_cast<float*>(cbuf.p);
        int rc;
        if ((rc = run_pair_f32(h, rb[0], rb[1], x3, x_dev, B, L, tT, ACC_STORE, 1.f, st))) return rc;
        if ((rc = run_pair_f32(h, rb[2], rb[3], x3, tT, B, L, tC, ACC_STORE, 1.f, st))) return rc;
        return run_pair_f32(h, rb[4], rb[5], x3, tC, B, L, y_dev, mode, div, st);
    }
    // bf16 handle: fp32 channels-last [B, L, C] in and out through bf16 buffers of the hook's own; synchronises (as run_pair)
    if (!(slope_out > 0.0f && slope_out <= 1.0f)) return failf(VTTS_ERR_INVALID, "run_resblock(): slope_out must lie in (0, 1] on a bf16 handle (got %g)", slope_out);
    if (route == 0 && !rb[0].has_rb) return failf(VTTS_ERR_INVALID, "'%s': no whole-ResBlock kernel for this ResBlock (C = 32; C = 64 / 128 at k = 3)", key_c1_0);
    if (route == 1 && !(rb[0].has_pair && rb[2].has_pair && rb[4].has_pair))
        return failf(VTTS_ERR_INVALID, "'%s': the fused pair kernel does not cover this ResBlock", key_c1_0);
    DevBuf xbuf, ybuf, tbuf, cbuf;
    HIP_TRY(hipMalloc(&xbuf.p, n * 2));
    HIP_TRY(hipMalloc(&ybuf.p, n * 2));
    if (route == 1) {
        HIP_TRY(hipMalloc(&tbuf.p, n * 2));
        HIP_TRY(hipMalloc(&cbuf.p, n * 2));
    }
    int rc = VTTS_OK;
    if (launch_f32_to_bf16(x_dev, xbuf.p, n, st) != hipSuccess || launch_f32_to_bf16(y_dev, ybuf.p, n, st) != hipSuccess)
        rc = failf(VTTS_ERR_HIP, "conversion launch failed");
    if (!rc && route == 0) rc = run_resblock_bf16(h, rb, xbuf.p, B, L, slope_out, ybuf.p, acc_add, div, st);
    if (!rc && route == 1) {  // X -> T -> C -> y, as mrf_bf16 (no tail)
        rc = run_pair_bf16(h, rb[0], xbuf.p, B, L, 1.0f, tbuf.p, 0, 1.f, st);
        if (!rc) rc = run_pair_bf16(h, rb[2], tbuf.p, B, L, 1.0f, cbuf.p, 0, 1.f, st);
        if (!rc) rc = run_pair_bf16(h, rb[4], cbuf.p, B, L, slope_out, ybuf.p, acc_add, div, st);
    }
    if (!rc && launch_bf16_to_f32(ybuf.p, y_dev, n, st) != hipSuccess) rc = failf(VTTS_ERR_HIP, "conversion launch failed");
    hipError_t e = hipStreamSynchronize(st);
    if (!rc && e != hipSuccess) rc = failf(VTTS_ERR_HIP, "run_resblock failed: %s", hipGetErrorString(e));
    return rc;
}

VTTS_API int vtts_hifigan_set_option(vtts_hifigan* h, const char* name, int64_t value) {
    if (!h || !name) return failf(VTTS_ERR_INVALID, "null argument");
    {  // setting a WRITABLE option to the value it has changes nothing: captured graphs stay valid (read-only and unknown names fall through to their errors)
        static const char* const writable[] = {"kernels", "microbatch", "fuse", "streams", "graph", "zigzag", "chains", "tiles", "tail", "upfuse", "stage"};
        for (const char* w : writable) {
            int64_t cur = 0;
            if (!strcmp(name, w) && vtts_hifigan_get_option(h, name, &cur) == VTTS_OK && cur == value) return VTTS_OK;
        }
    }
    ++h->epoch;  // a captured launch sequence reflects the options it was captured under
    if (!strcmp(name, "kernels")) {
        if (value != 0 && value != 1) return failf(VTTS_ERR_INVALID, "kernels must be 0 (auto) or 1 (generic)");
        h->opt_kernels = value;
    } else if (!strcmp(name, "microbatch")) {
        if (value < 0) return failf(VTTS_ERR_INVALID, "microbatch must be >= 0");
        h->opt_microbatch = value;
    } else if (!strcmp(name, "fuse")) {
        if (value < 0 || value > 3) return failf(VTTS_ERR_INVALID, "fuse must be 0 (per convolution), 1 (pairs), 2 (bf16: pairs + whole ResBlocks where faster; fp32: pairs at C <= 64) or 3 (... wherever supported)");
        h->opt_fuse = value;
    } else if (!strcmp(name, "streams")) {
        if (value < 0 || value > 4) return failf(VTTS_ERR_INVALID, "streams must be 1..4 (0 = the engine's default)");
        h->opt_streams = value;
    } else if (!strcmp(name, "graph")) {
        if (value != 0 && value != 1) return failf(VTTS_ERR_INVALID, "graph must be 0 (always eager) or 1 (small launches replay a captured hipGraph)");
        h->opt_graph = value;
    } else if (!strcmp(name, "zigzag")) {
        if (value != 0 && value != 1) return failf(VTTS_ERR_INVALID, "zigzag must be 0 or 1");
        h->opt_zigzag = value;
    } else if (!strcmp(name, "chains")) {
        if (value < 0 || value > 2) return failf(VTTS_ERR_INVALID, "chains must be 0 (ResBlocks of a stage one after the other), 1 (side by side on small fp32 launches) or 2 (... on every single-micro-batch launch)");
        h->opt_chains = value;
    } else if (!strcmp(name, "tiles")) {
        if (value < 0 || value > 2) return failf(VTTS_ERR_INVALID, "tiles must be 0 (auto), 1 (wide) or 2 (narrow)");
        h->opt_tiles = value;
    } else if (!strcmp(name, "tail")) {
        if (value != 0 && value != 1) return failf(VTTS_ERR_INVALID, "tail must be 0 or 1");
        h->opt_tail = value;
    } else if (!strcmp(name, "upfuse")) {
        if (value < 0 || value > 3) return failf(VTTS_ERR_INVALID, "upfuse must be 0..3 (bit 0: ups_2, bit 1: ups_3 inside the pair launch that ends the stage before it)");
        h->opt_upfuse = value;
    } else if (!strcmp(name, "stage")) {  // kept for callers that still set it: 0 is the only path there is
        if (value != 0) return failf(VTTS_ERR_INVALID, "stage must be 0: the whole-stage kernel was removed (it measured slower, profiles/r06_a_stage_kernel_findings.md)");
    } else if (!strcmp(name, "profile")) {
        h->opt_profile = value ? 1 : 0;
    } else if (!strcmp(name, "hop") || !strcmp(name, "pass_frames") || !strcmp(name, "max_frames_per_pass") || !strcmp(name, "graphs_cached") ||
               !strcmp(name, "profile_C") || !strcmp(name, "profile_K")) {
        return failf(VTTS_ERR_INVALID, "option '%s' is read-only", name);
    } else {
        return failf(VTTS_ERR_INVALID, "unknown option '%s'", name);
    }
    return VTTS_OK;
}

VTTS_API int vtts_hifigan_get_option(const vtts_hifigan* h, const char* name, int64_t* value) {
    if (!h || !name || !value) return failf(VTTS_ERR_INVALID, "null argument");
    if (!strcmp(name, "kernels")) *value = h->opt_kernels;
    else if (!strcmp(name, "microbatch")) *value = h->opt_microbatch;
    else if (!strcmp(name, "profile")) *value = h->opt_profile;
    else if (!strcmp(name, "tiles")) *value = h->opt_tiles;
    else if (!strcmp(name, "streams")) *value = h->opt_streams;
    else if (!strcmp(name, "zigzag")) *value = h->opt_zigzag;
    else if (!strcmp(name, "chains")) *value = h->opt_chains;
    else if (!strcmp(name, "graph")) *value = h->opt_graph;
    else if (!strcmp(name, "tail")) *value = h->opt_tail;
    else if (!strcmp(name, "upfuse")) *value = h->opt_upfuse;
    else if (!strcmp(name, "stage")) *value = 0;
    else if (!strcmp(name, "graphs_cached")) {
        *value = 0;
        for (auto& g : h->graphs) *value += g.exec ? 1 : 0;
    }
    else if (!strcmp(name, "fuse")) *value = h->opt_fuse;
    else if (!strcmp(name, "hop")) *value = h->hop;
    else if (!strcmp(name, "max_frames_per_pass")) {
        // the smallest T check_pass_size() refuses (one utterance's largest activation must stay below 2^31 bytes; max_act_elems is linear
        // in T): callers route longer utterances through the chunk scheduler — ONE rule, here
        const size_t per = max_act_elems(h, 1) * elem_bytes(h);
        *value = (int64_t)((((size_t)1 << 31) + per - 1) / per);
    }
    else if (!strcmp(name, "pass_frames")) *value = pass_frames(h);
    else if (!strcmp(name, "profile_C")) *value = h->prof_C;
    else if (!strcmp(name, "profile_K")) *value = h->prof_K;
    else return failf(VTTS_ERR_INVALID, "unknown option '%s'", name);
    return VTTS_OK;
}

VTTS_API int vtts_hifigan_profile_read(vtts_hifigan* h, double* resblock_ms, int64_t* launches, double* resblock_flops,
                                       int reset) {
    if (!h) return failf(VTTS_ERR_INVALID, "null argument");
    double ms = 0.0;
    for (size_t i = 0; i < h->prof_used; ++i) {
        float t = 0.f;
        HIP_TRY(hipEventSynchronize(h->prof_events[i].second));
        HIP_TRY(hipEventElapsedTime(&t, h->prof_events[i].first, h->prof_events[i].second));
        ms += t;
    }
    if (resblock_ms) *resblock_ms = ms;
    if (launches) *launches = (int64_t)h->prof_used;
    if (resblock_flops) *resblock_flops = h->prof_flops;
    if (reset) {
        h->prof_used = 0;
        h->prof_flops = 0.0;
    }
    return VTTS_OK;
}

VTTS_API const char* vtts_hifigan_profile_kernel(const vtts_hifigan* h) {
    if (!h) return "";
    return (h->dtype == VTTS_BF16 && h->opt_fuse) ? h->prof_name_pair.c_str() : h->prof_name.c_str();
}
