// Host side of the NAT models' parameters (nat.hip): the arrays a model takes from the checkpoint, the packed device blob, and the kernels'
// private weight layouts.  Host code only; pack()'s upload is the one place that needs the HIP runtime.
#pragma once

#include <cmath>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include "vtts_internal.h"

namespace vtts {

// round-to-nearest-even bf16 of a float (host side of the bf16x3 split: v0 = bf16(v), v1 = bf16(v - v0); v - v0 is exact in fp32)
inline unsigned short nat_bf16_rne(float v) {
    uint32_t u;
    memcpy(&u, &v, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (unsigned short)((u >> 16) | 0x40);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (unsigned short)(u >> 16);
}
inline float nat_bf16_to_float(unsigned short h) {
    const uint32_t u = (uint32_t)h << 16;
    float f;
    memcpy(&f, &u, 4);
    return f;
}
// the split fragments keep a lane group's 64 x 8 hi terms in front of its lo terms
inline void nat_store_x3(unsigned short* out, size_t i, float w) {
    out[i] = nat_bf16_rne(w);
    out[i + 64 * 8] = nat_bf16_rne(w - nat_bf16_to_float(out[i]));
}

// The LSTM step kernels' accumulator order of an hk.LSTM's 4H gate columns, as a table [c'] -> Haiku column:
// c' = ((slice * 2 + lane / 32) * 4 + unit pair) * 4 + gate  <->  gate * H + 8 * slice + 2 * (unit pair) + lane / 32
inline std::vector<int> nat_hcol(int H) {
    std::vector<int> t(4 * (size_t)H);
    for (int cp = 0; cp < 4 * H; ++cp) t[cp] = (cp & 3) * H + 8 * (cp >> 5) + 2 * ((cp >> 2) & 3) + ((cp >> 4) & 1);
    return t;
}

// ---- convolution / GEMM weights as MFMA A fragments (nat_conv_mfma_k, nat_conv_x3_k) ----
// W = [taps][cin][ncols] (Haiku's Conv1D order; a Linear's [rows][ncols] is one tap), of which the fragments take rows [row0, row0 + cin) and the
// `cout` columns col[co] (col = nullptr: co itself), zero-padded to multiples of 32 both ways.  fp32: [mblk][32-channel step][tap][lane][16],
// element e of lane = W[tap][row0 + 32 * step + 16 * (lane / 32) + e][col[32 * mblk + lane % 32]].
inline size_t nat_conv_frag_bytes(int taps, int cin, int cout) { return (size_t)((cout + 31) / 32) * ((cin + 31) / 32) * taps * 64 * 16 * sizeof(float); }
inline float nat_conv_frag_w(const float* W, int j, int c, int co, int row0, int cin, int cout, int ncols, const int* col) {
    return (c < cin && co < cout) ? W[((size_t)j * cin + row0 + c) * ncols + (col ? col[co] : co)] : 0.0f;
}
inline void pack_conv_frag_f32(const float* W, int taps, int row0, int cin, int cout, int ncols, const int* col, float* out) {
    const int MB = (cout + 31) / 32, NCS = (cin + 31) / 32;
    for (int mb = 0; mb < MB; ++mb)
        for (int cs = 0; cs < NCS; ++cs)
            for (int j = 0; j < taps; ++j)
                for (int lane = 0; lane < 64; ++lane)
                    for (int e = 0; e < 16; ++e)
                        out[((((size_t)mb * NCS + cs) * taps + j) * 64 + lane) * 16 + e] =
                            nat_conv_frag_w(W, j, 32 * cs + 16 * (lane >> 5) + e, 32 * mb + (lane & 31), row0, cin, cout, ncols, col);
}
// ... and split into two bf16 terms: [mblk][step][tap][16-channel half][hi | lo][lane][8] bf16 (as many bytes), element e of lane = the term of
// W[tap][row0 + 32 * step + 16 * half + 8 * (lane / 32) + e][col[32 * mblk + lane % 32]]
inline void pack_conv_frag_x3(const float* W, int taps, int row0, int cin, int cout, int ncols, const int* col, unsigned short* out) {
    const int MB = (cout + 31) / 32, NCS = (cin + 31) / 32;
    for (int mb = 0; mb < MB; ++mb)
        for (int cs = 0; cs < NCS; ++cs)
            for (int j = 0; j < taps; ++j)
                for (int ks = 0; ks < 2; ++ks)
                    for (int lane = 0; lane < 64; ++lane)
                        for (int e = 0; e < 8; ++e)
                            nat_store_x3(out, (((((size_t)mb * NCS + cs) * taps + j) * 4 + ks * 2) * 64 + lane) * 8 + e,
                                         nat_conv_frag_w(W, j, 32 * cs + 16 * ks + 8 * (lane >> 5) + e, 32 * mb + (lane & 31), row0, cin, cout, ncols, col));
}

// ---- rows [row0, row0 + K) of an hk.LSTM's [.][4H] matrix as MFMA A fragments for the step kernels ----
// fp32 (nat_dec_lstm_k, nat_tf_lstm_k): [slice = 8 units][K / 8][lane][4], element i of lane = W[row0 + 8 * kb + 4 * (lane / 32) + i][gate * H + 8 * slice + unit],
// (unit, gate) = ((lane % 32) / 4, (lane % 32) % 4)
inline size_t nat_lstm_frag_bytes(int K, int H) { return (size_t)K * 4 * H * sizeof(float); }
inline void pack_lstm_frag_f32(const float* W, int K, int H, int row0, float* out) {
    const int NIT = K / 8;
    for (int sl = 0; sl < H / 8; ++sl)
        for (int kb = 0; kb < NIT; ++kb)
            for (int lane = 0; lane < 64; ++lane) {
                const int mrow = lane & 31, lh = lane >> 5, col = (mrow & 3) * H + 8 * sl + (mrow >> 2);
                for (int i = 0; i < 4; ++i) out[(((size_t)sl * NIT + kb) * 64 + lane) * 4 + i] = W[(size_t)(row0 + 8 * kb + 4 * lh + i) * 4 * H + col];
            }
}
// ... and split into two bf16 terms (nat_dec_lstm_x3_k): [slice][K / 16][hi | lo][lane][8] bf16 (as many bytes), element i of lane = the term of
// W[row0 + 16 * step + 8 * (lane / 32) + i][gate * H + 8 * slice + unit]
inline void pack_lstm_frag_x3(const float* W, int K, int H, int row0, unsigned short* out) {
    const int NST = K / 16;
    for (int sl = 0; sl < H / 8; ++sl)
        for (int st = 0; st < NST; ++st)
            for (int lane = 0; lane < 64; ++lane) {
                const int mrow = lane & 31, lh = lane >> 5, col = (mrow & 3) * H + 8 * sl + (mrow >> 2);
                for (int i = 0; i < 8; ++i) nat_store_x3(out, ((((size_t)sl * NST + st) * 2) * 64 + lane) * 8 + i, W[(size_t)(row0 + 16 * st + 8 * lh + i) * 4 * H + col]);
            }
}

struct Arr {
    std::string module, name;
    std::vector<int64_t> shape;
    std::vector<float> host;
    bool have = false;
    size_t off = 0;  // byte offset in the packed blob
    size_t elems() const {
        size_t n = 1;
        for (auto d : shape) n *= (size_t)d;
        return n;
    }
};

// Arrays a model takes from the checkpoint (Haiku module tail + array name), their place in the packed device blob, and
// the derived per-BatchNorm vectors inv = scale * rsqrt(var + eps) appended behind them.
struct NatModel {
    const char* what = "model";
    int device = 0;
    std::vector<Arr> arrs;
    std::vector<std::pair<std::string, int>> bns;  // (BatchNorm module tail, channels)
    std::vector<size_t> bn_off;
    struct Extra {  // a kernel-private re-layout of checkpoint arrays, built at image() time behind the plain arrays
        std::string key;
        size_t bytes = 0, off = 0;
        std::function<void(const NatModel&, void*)> fill;
    };
    std::vector<Extra> extras;
    size_t blob_bytes = 0;
    char* blob = nullptr;

    void add(const std::string& m, const char* n, std::vector<int64_t> shp) { arrs.push_back(Arr{m, n, std::move(shp)}); }
    void add_bn(const std::string& m, int C) {
        add(m, "scale", {1, 1, C});
        add(m, "offset", {1, 1, C});
        add(m + "/~/mean_ema", "average", {1, 1, C});
        add(m + "/~/var_ema", "average", {1, 1, C});
        bns.emplace_back(m, C);
    }
    // TokenEncoder (model.py:12-24): Embed, 3 x (Conv1D k=3 + BatchNorm), forward LSTM, backward LSTM
    void add_token_encoder(const std::string& te, int V, int D) {
        add(te + "embed", "embeddings", {V, D});
        for (int i = 0; i < 3; ++i) {
            const std::string sfx = i ? "_" + std::to_string(i) : "";
            add(te + "conv1_d" + sfx, "w", {3, D, D});
            add(te + "conv1_d" + sfx, "b", {D});
            add_bn(te + "batch_norm" + sfx, D);
        }
        for (const char* l : {"lstm/linear", "lstm_1/linear"}) {
            add(te + l, "w", {2 * D, 4 * D});
            add(te + l, "b", {4 * D});
            add_lstm_frag(te + l + "#mfma", te + l, false, 2 * D, D, 0);  // rows [x ; h] as hk.LSTM concatenates them
        }
    }
    void add_extra(const std::string& key, size_t bytes, std::function<void(const NatModel&, void*)> fill) { extras.push_back(Extra{key, bytes, 0, std::move(fill)}); }
    // module `mod`'s "w" through one of the packers above (x3: its bf16 split)
    void add_conv_frag(const std::string& key, const std::string& mod, bool x3, int taps, int row0, int cin, int cout, int ncols, std::vector<int> col = {}) {
        add_extra(key, nat_conv_frag_bytes(taps, cin, cout), [=](const NatModel& m, void* out) {
            const int* cm = col.empty() ? nullptr : col.data();
            if (x3) pack_conv_frag_x3(m.host(mod, "w"), taps, row0, cin, cout, ncols, cm, static_cast<unsigned short*>(out));
            else pack_conv_frag_f32(m.host(mod, "w"), taps, row0, cin, cout, ncols, cm, static_cast<float*>(out));
        });
    }
    void add_lstm_frag(const std::string& key, const std::string& mod, bool x3, int K, int H, int row0) {
        add_extra(key, nat_lstm_frag_bytes(K, H), [=](const NatModel& m, void* out) {
            if (x3) pack_lstm_frag_x3(m.host(mod, "w"), K, H, row0, static_cast<unsigned short*>(out));
            else pack_lstm_frag_f32(m.host(mod, "w"), K, H, row0, static_cast<float*>(out));
        });
    }
    void add_zeros(const std::string& key, int n) {  // (the image is zero-filled)
        add_extra(key, (size_t)n * sizeof(float), [](const NatModel&, void*) {});
    }
    template <class T = float>
    const T* extra(const std::string& key) const {
        for (auto& e : extras)
            if (e.key == key) return reinterpret_cast<const T*>(blob + e.off);
        return nullptr;
    }
    void layout() {
        size_t off = 0;
        for (auto& a : arrs) {
            a.off = off;
            off = align_up(off + a.elems() * sizeof(float), 256);
        }
        for (auto& b : bns) {
            bn_off.push_back(off);
            off = align_up(off + (size_t)b.second * sizeof(float), 256);
        }
        for (auto& e : extras) {
            e.off = off;
            off = align_up(off + e.bytes, 256);
        }
        blob_bytes = off;
    }
    int find(const std::string& module, const char* name) const {
        for (size_t i = 0; i < arrs.size(); ++i)
            if (arrs[i].module == module && arrs[i].name == name) return (int)i;
        return -1;
    }
    const float* host(const std::string& module, const char* name) const { return arrs[find(module, name)].host.data(); }
    const float* dev(const std::string& module, const char* name) const { return reinterpret_cast<const float*>(blob + arrs[find(module, name)].off); }
    const float* inv(const std::string& bn) const {
        for (size_t i = 0; i < bns.size(); ++i)
            if (bns[i].first == bn) return reinterpret_cast<const float*>(blob + bn_off[i]);
        return nullptr;
    }

    int param_info(int i, const char** module, const char** name, int64_t shape[3], int* ndim) const {
        if (i < 0 || i >= (int)arrs.size()) return failf(VTTS_ERR_INVALID, "parameter index out of range");
        const Arr& a = arrs[i];
        if (module) *module = a.module.c_str();
        if (name) *name = a.name.c_str();
        if (shape)
            for (int d = 0; d < 3; ++d) shape[d] = d < (int)a.shape.size() ? a.shape[d] : 1;
        if (ndim) *ndim = (int)a.shape.size();
        return VTTS_OK;
    }
    int set_param(const char* module, const char* name, const float* host, const int64_t* shape, int ndim) {
        if (!module || !name || !host || !shape) return failf(VTTS_ERR_INVALID, "null argument");
        const int i = find(module, name);
        if (i < 0) return failf(VTTS_ERR_INVALID, "%s has no array '%s' in module '%s'", what, name, module);
        Arr& a = arrs[i];
        if (ndim != (int)a.shape.size()) return failf(VTTS_ERR_SHAPE, "%s/%s: expected %zu dimensions, got %d", module, name, a.shape.size(), ndim);
        for (int d = 0; d < ndim; ++d)
            if (shape[d] != a.shape[d])
                return failf(VTTS_ERR_SHAPE, "%s/%s: dimension %d is %lld, expected %lld", module, name, d, (long long)shape[d], (long long)a.shape[d]);
        a.host.assign(host, host + a.elems());
        a.have = true;
        return VTTS_OK;
    }
    // the blob's bytes on the host: needs no device
    int image(std::vector<char>& img) const {
        for (auto& a : arrs)
            if (!a.have) return failf(VTTS_ERR_MISSING, "array %s/%s was never set", a.module.c_str(), a.name.c_str());
        img.assign(blob_bytes, 0);
        for (auto& a : arrs) memcpy(img.data() + a.off, a.host.data(), a.elems() * sizeof(float));
        for (size_t i = 0; i < bns.size(); ++i) {
            const float *sc = host(bns[i].first, "scale"), *var = host(bns[i].first + "/~/var_ema", "average");
            float* iv = reinterpret_cast<float*>(img.data() + bn_off[i]);
            for (int c = 0; c < bns[i].second; ++c) iv[c] = sc[c] / std::sqrt(var[c] + 1e-5f);  // hk.BatchNorm eps
        }
        for (auto& e : extras) e.fill(*this, img.data() + e.off);
        return VTTS_OK;
    }
    int pack(void* dev_blob, size_t bytes, void* stream) {
        if (int rc = check_blob(dev_blob, bytes, blob_bytes)) return rc;
        std::vector<char> img;
        if (int rc = image(img)) return rc;
        if (int rc = upload_blob(dev_blob, img.data(), blob_bytes, static_cast<hipStream_t>(stream), "the model's weights")) return rc;
        blob = static_cast<char*>(dev_blob);
        return VTTS_OK;
    }
    int bind(void* dev_blob, size_t bytes) {
        if (int rc = check_blob(dev_blob, bytes, blob_bytes)) return rc;
        blob = static_cast<char*>(dev_blob);
        return VTTS_OK;
    }
};

}  // namespace vtts
