/*
 * vtts_nat.h — C ABI of the MI355X-native NAT duration and acoustic models of NTT123/vietTTS (the caller-side rows
 * next to the mel->waveform hot path: they decide how many mel frames mel2wave() will see, and produce them).
 *
 * Entry points a maintainer of the reference would bind (ctypes stub in INTEGRATION.md) to replace the body of
 *     vietTTS/nat/text2mel.py:22-34   predict_duration(tokens)
 * i.e. "load duration_latest_ckpt.pickle, build DurationModel(is_training=False), apply it to the token ids"
 * (vietTTS/nat/model.py:9-70).  Same conventions as vtts_hifigan.h: plain pointers and sizes, 0 / negative
 * vtts_status (message via vtts_last_error()), device memory owned by the caller, asynchronous on the given stream.
 */
#ifndef VTTS_NAT_H
#define VTTS_NAT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* vietTTS/nat/config.py:11-13: the fields DurationModel.__init__ / TokenEncoder.__init__ read. */
typedef struct vtts_nat_duration_cfg {
    int32_t vocab_size;        /* 256 */
    int32_t lstm_dim;          /* 256: embedding width = conv channels = LSTM units */
} vtts_nat_duration_cfg;

typedef struct vtts_nat_duration vtts_nat_duration; /* opaque */

/* Replaces: DurationModel(is_training=False) construction, vietTTS/nat/model.py:56-66 (via text2mel.py:23-26). */
int vtts_nat_duration_create(const vtts_nat_duration_cfg* cfg, int device, vtts_nat_duration** out);
void vtts_nat_duration_destroy(vtts_nat_duration* h);

/*
 * Supply one array of the checkpoint (text2mel.py:27-28: dic["params"] and dic["aux"]) by the TAIL of its Haiku
 * module path and its name inside that module, e.g.
 *   ("token_encoder/~/embed", "embeddings") [V,D]      ("token_encoder/~/conv1_d_2", "w") [3,D,D] / "b" [D]
 *   ("token_encoder/~/batch_norm_1", "scale" | "offset") [1,1,D]
 *   ("token_encoder/~/batch_norm_1/~/mean_ema" | ".../~/var_ema", "average") [1,1,D]     (state)
 *   ("token_encoder/~/lstm/linear" | "token_encoder/~/lstm_1/linear", "w") [2D,4D] / "b" [4D]   (forward | backward)
 *   ("linear", "w") [2D,D] / "b" [D]        ("linear_1", "w") [D,1] / "b" [1]
 * fp32 host memory, copied before return.  num_params()/param_info() enumerate what is expected.
 */
int vtts_nat_duration_set_param(vtts_nat_duration* h, const char* module, const char* name, const float* host,
                                const int64_t* shape, int ndim);
int vtts_nat_duration_num_params(const vtts_nat_duration* h, int* n);
int vtts_nat_duration_param_info(const vtts_nat_duration* h, int i, const char** module, const char** name,
                                 int64_t shape[3], int* ndim);

/* Packed device blob (caller-owned, 256-B aligned), as in vtts_hifigan.h.  pack() and bind_packed() of both models refuse a misaligned
 * blob with VTTS_ERR_INVALID, as every other handle does: the kernels read the blob as float4 / uint4. */
int vtts_nat_duration_packed_bytes(const vtts_nat_duration* h, size_t* bytes);
int vtts_nat_duration_pack(vtts_nat_duration* h, void* dev_blob, size_t blob_bytes, void* stream);
int vtts_nat_duration_bind_packed(vtts_nat_duration* h, void* dev_blob, size_t blob_bytes);

/* Scratch bytes forward() needs for B sentences of at most Lmax tokens. */
int vtts_nat_duration_workspace_bytes(const vtts_nat_duration* h, int B, int Lmax, size_t* bytes);

/*
 * Replaces forward_fn(params, aux, rng, DurationInput(tokens[None], [len], None))[0], text2mel.py:29-34 ==
 * DurationModel.__call__, model.py:68-70, one sentence per row (the reference runs batch 1; rows are independent):
 *   tokens_dev    [B, Lmax] int32 token ids (text2tokens, text2mel.py:37-58); entries past a row's length are ignored
 *   lengths_dev   [B] int32, 1 <= length <= Lmax
 *   durations_dev [B, Lmax] fp32 seconds per token; entries past a row's length are set to 0
 */
int vtts_nat_duration_forward(vtts_nat_duration* h, const int32_t* tokens_dev, const int32_t* lengths_dev, int B, int Lmax,
                              float* durations_dev, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Acoustic model: replaces predict_mel()'s network apply, vietTTS/nat/text2mel.py:61-82 ==
 * AcousticModel(is_training=False).inference(tokens, durations, n_frames), vietTTS/nat/model.py:128-151.
 * ------------------------------------------------------------------------------------------------------------------ */
typedef struct vtts_nat_acoustic_cfg { /* vietTTS/nat/config.py:11-17, :42; model.py:88-89.  The reference's value, then what create() accepts
                                        * (anything else is VTTS_ERR_INVALID with a message naming the rule; no forward*() refuses a width create() accepted) */
    int32_t vocab_size;   /* 256; >= 1 */
    int32_t encoder_dim;  /* acoustic_encoder_dim 256; 64, 128, 192 or 256 */
    int32_t decoder_dim;  /* acoustic_decoder_dim 512; 256, 512, 768 or 1024 (the gate mix takes 4 * decoder_dim columns in chunks of 1024) */
    int32_t prenet_dim;   /* 256 (hk.Linear(256) x 2); a multiple of 32 with 2 * encoder_dim + prenet_dim <= 1024 */
    int32_t mel_dim;      /* 80; a multiple of 4 in 4 .. 128 */
    int32_t postnet_dim;  /* 512; a multiple of 4 in 4 .. 1024 */
} vtts_nat_acoustic_cfg;

typedef struct vtts_nat_acoustic vtts_nat_acoustic; /* opaque */

int vtts_nat_acoustic_create(const vtts_nat_acoustic_cfg* cfg, int device, vtts_nat_acoustic** out);
void vtts_nat_acoustic_destroy(vtts_nat_acoustic* h);
/* Arrays by Haiku module tail under "acoustic_model/~/": "token_encoder/~/..." as above; "lstm/linear", "lstm_1/linear"
 * (decoder layers), "linear" (mel projection), "linear_1" / "linear_2" (prenet, "w" only), "conv1_d" .. "conv1_d_4" and
 * "batch_norm" .. "batch_norm_3" (+ "/~/mean_ema", "/~/var_ema" state) of the postnet. */
int vtts_nat_acoustic_set_param(vtts_nat_acoustic* h, const char* module, const char* name, const float* host,
                                const int64_t* shape, int ndim);
int vtts_nat_acoustic_num_params(const vtts_nat_acoustic* h, int* n);
int vtts_nat_acoustic_param_info(const vtts_nat_acoustic* h, int i, const char** module, const char** name,
                                 int64_t shape[3], int* ndim);
int vtts_nat_acoustic_packed_bytes(const vtts_nat_acoustic* h, size_t* bytes);
int vtts_nat_acoustic_pack(vtts_nat_acoustic* h, void* dev_blob, size_t blob_bytes, void* stream);
int vtts_nat_acoustic_bind_packed(vtts_nat_acoustic* h, void* dev_blob, size_t blob_bytes);
/* (Independent of the options: a workspace sized once serves every path.) */
int vtts_nat_acoustic_workspace_bytes(const vtts_nat_acoustic* h, int B, int Lmax, int Fmax, size_t* bytes);
/* Options (defaults in brackets):
 *   "bf16x3" [0]  1 = the matrix products of the decoder's LSTM steps, of the gate GEMM and of the postnet as three bf16 x bf16 terms on the
 *                 bf16 matrix pipe (every operand v = v0 + v1, v0 = bf16(v), v1 = bf16(v - v0); x * w ~ x1 w0 + x0 w1 + x0 w0, fp32
 *                 accumulation; the decoder state is kept split, the cell states, the projection and the prenet stay fp32): the mel moves
 *                 by ~1e-5 of its range (tests/test_gpu_nat.py) and the acoustic model runs a third faster.  The default keeps every
 *                 product in fp32 — the mode the parity tests against the reference pin at 5e-5.  For callers whose vocoder is
 *                 bf16-class anyway.  The token encoders and the duration model are fp32 in both modes (integer frame counts).
 *   "resident" [0]  1 = forward() and forward_from_encoder(ngroups = 0) run the decoder's frame loop as ONE resident kernel (nat_dec_resident_k: a
 *                 cooperative launch of one workgroup per CU that keeps the two LSTMs' recurrent weights in registers for all Fmax frames and
 *                 exchanges the state through agent-scope stores and loads between grid barriers, five per frame) instead of three launches per
 *                 frame — the low-latency path for one to four sentences.  It is taken when ALL of these hold: 1 <= B <= 4; "bf16x3" is 0; the
 *                 stream is not being captured; decoder_dim = 512, prenet_dim = 256 (the reference's; the kernel is built for them); the runtime
 *                 accepts the cooperative launch.  In every other case (B > 4, forward_groups(), ngroups >= 1, bf16x3, capture, other dimensions,
 *                 hipErrorCooperativeLaunchTooLarge, forward_teacher()) the call takes the per-frame launches, silently.  fp32 throughout; a row's
 *                 mel does not depend on its batch and runs repeat bit for bit, but the sums' order is this kernel's own: against the default path
 *                 the mel differs by fp32 rounding (both are pinned to the oracle by the same bar, tests/test_gpu_nat_resident.py).
 *                 Every wait inside the kernel is bounded (100 ms): see vtts_nat_acoustic_resident_status().
 *   "resident_grid" [0]  workgroups of the resident kernel: 64, 128 or 256; 0 = the library's default, halved
 *                 until it fits the device's CU count.  The result does not depend on it, bit for bit.  For measurements.
 *   "resident_used"  read-only (get_option): 1 if the handle's last forward took the resident kernel, else 0.
 *   "stage_times" [0]  1 = forward() / forward_from_encoder(ngroups = 0) record timing events on the stream in front of the gate GEMM, of the decoder's
 *                 frame loop, of the postnet and behind it; after the caller has synchronised, get_option reads "stage_gates_us" (token-rows GEMM + mix;
 *                 on the default path only the first 64 frames' mix, the rest runs beside the loop), "stage_decoder_us" and "stage_postnet_us" of the
 *                 last such call in whole microseconds (VTTS_ERR_STATE if there was none).  For tools/latency_bench.py.
 * Unknown keys and out-of-range values return VTTS_ERR_INVALID. */
int vtts_nat_acoustic_set_option(vtts_nat_acoustic* h, const char* key, int value);
int vtts_nat_acoustic_get_option(const vtts_nat_acoustic* h, const char* key, int* value);
/*
 * After the caller has synchronised the stream of a forward that took the resident kernel: *timed_out = 1 if a wait inside the handle's last
 * resident launch exceeded its budget (100 ms of the device's wall clock, four orders of magnitude above a barrier) — every workgroup then
 * left the kernel and the frames not produced are zero in mel_dev — else 0.  A synchronous 8-byte copy from the workspace of that call, which
 * must still be allocated.  VTTS_ERR_STATE if the handle has not launched the resident kernel.
 */
int vtts_nat_acoustic_resident_status(vtts_nat_acoustic* h, int* timed_out);
/*
 *   tokens_dev    [B, Lmax] int32, lengths_dev [B] int32                       as for the duration model
 *   durations_dev [B, Lmax] fp32, in FRAMES (text2mel.py:78: seconds * sample_rate / hop)
 *   nframes_dev   [B] int32: frames to generate per sentence (text2mel.py:79), <= Fmax
 *   keep_dev      [B, Fmax, 2, prenet_dim] bytes: the prenet's two dropout KEEP masks per frame (1 = keep and scale by 2;
 *                 model.py:95-100 — dropout is on at inference), or NULL for no dropout.  The reference draws them from
 *                 JAX's threefry PRNG through Haiku's per-scan-step key splitting; that stream is the caller's business.
 *   mel_dev       [B, Fmax, mel_dim] fp32 log-mel (decoder output + postnet residual); rows past nframes are zero
 */
/*
 * Draws keep masks for forward() on the device: keep_dev [B, Fmax, 2, prenet_dim] bytes, P(keep) = 1/2 (hk.dropout(key,
 * 0.5, x), model.py:97,:99), from seeds_dev [B] (one 64-bit seed per sentence, so a sentence's masks do not depend on
 * the batch it is in) with Threefry-2x32-20: key = seed, counter = (2 * frame + layer, 64-column block), output bit j =
 * column 64 * block + j.  The cipher is the one jax.random uses; the STREAM is this library's own (per-sentence seeds:
 * independent of batching, which a throughput pipeline wants) — the reference's own stream is the next entry point.
 */
int vtts_nat_acoustic_keep_masks(const vtts_nat_acoustic* h, const uint64_t* seeds_dev, int B, int Fmax, uint8_t* keep_dev, void* stream);
/*
 * The same masks as the REFERENCE draws them (text2mel.py:65-73 -> model.py:95-100,134-142): (rng_key0, rng_key1) = the
 * checkpoint's `rng` (a jax.random.PRNGKey, uint32[2]); dm-haiku's PRNGSequence hands out S_n of the chain
 * (K_n, S_n) = jax.random.split(K_{n-1}), frame f takes S_{2f+1} and S_{2f+2}, a mask is
 * jax.random.bernoulli(S, 0.5, (1, prenet_dim)) on jax.random's classic (pre-0.5 default, non-"partitionable") threefry
 * layout.  Every sentence of the batch gets the same masks, as every run of the reference starts from the same key.
 * Restatement: oracle/nat_oracle.py::haiku_prenet_keep_masks (pinned by the known answers JAX's documentation prints for
 * PRNGKey(0); not by a JAX run: none is possible offline).  A checkpoint run under JAX >= 0.5 defaults draws another stream.
 */
int vtts_nat_acoustic_keep_masks_haiku(const vtts_nat_acoustic* h, uint32_t rng_key0, uint32_t rng_key1, int B, int Fmax, uint8_t* keep_dev,
                                       void* stream);
/*
 * ... with the threefry layout as a parameter: threefry_partitionable = 0 is the entry point above; 1 is the layout JAX >= 0.5 uses by
 * default (jax_threefry_partitionable=True: subkey i of a split and element c of a 32-bit draw are the cipher on the 64-bit index
 * itself, a draw's word = y0 ^ y1).  The reference pins no JAX version (setup.py:6-19), so which stream a given checkpoint was
 * sampled with at inference depends on the JAX it ran under.  Mode 1 is restated from recollection of jax/_src/prng.py
 * (oracle/nat_oracle.py::jax_partitionable_*) and is NOT pinned by any known answer: use it knowingly.
 */
int vtts_nat_acoustic_keep_masks_haiku_mode(const vtts_nat_acoustic* h, uint32_t rng_key0, uint32_t rng_key1, int threefry_partitionable, int B,
                                            int Fmax, uint8_t* keep_dev, void* stream);
int vtts_nat_acoustic_forward(vtts_nat_acoustic* h, const int32_t* tokens_dev, const int32_t* lengths_dev,
                              const float* durations_dev, const int32_t* nframes_dev, int B, int Lmax, int Fmax,
                              const uint8_t* keep_dev, float* mel_dev, void* workspace, size_t workspace_bytes, void* stream);
/*
 * forward() that hands the mel over in GROUPS of rows as the decoder finishes them (the text -> waveform pipeline, BASELINE configs[3];
 * the reference synthesises one sentence per process, vietTTS/synthesizer.py:33-39, and has nothing to overlap).  The decoder is a chain
 * of Fmax dependent steps that barely loads the chip; a sentence's mel is complete after ITS last frame, long before the batch's.
 *   group_row0   HOST [ngroups + 1]: group g = rows [group_row0[g], group_row0[g + 1]); group_row0[0] = 0, group_row0[ngroups] = B
 *   group_frames HOST [ngroups]: the largest nframes among the group's rows (1 .. Fmax)
 * The arithmetic of every row is that of forward() (same kernels, same order: bit-identical mel).  After decoder frame
 * group_frames[g] - 1 the group's postnet runs on a stream of the handle's own beside the remaining decoder steps, and
 * vtts_nat_acoustic_wait_group(h, g, consumer_stream) makes `consumer_stream` wait for exactly that (rows of group g of mel_dev
 * complete) — e.g. the stream a vocoder runs on.  `stream` itself waits for every group before the call's work on it ends, so code
 * that ignores the groups sees forward()'s semantics.  Sort the rows by descending nframes to make the groups finish one after another.
 */
int vtts_nat_acoustic_forward_groups(vtts_nat_acoustic* h, const int32_t* tokens_dev, const int32_t* lengths_dev,
                                     const float* durations_dev, const int32_t* nframes_dev, int B, int Lmax, int Fmax,
                                     const uint8_t* keep_dev, float* mel_dev, void* workspace, size_t workspace_bytes, void* stream,
                                     int ngroups, const int32_t* group_row0, const int32_t* group_frames);
/*
 * The TEACHER-FORCED pass: AcousticModel(is_training=False).__call__, vietTTS/nat/model.py:146-169 — what vietTTS/nat/gta.py:28-40 runs over a
 * corpus to dump ground-truth-aligned mels for the vocoder's fine-tuning.  tokens / lengths / durations (FRAMES, fp32, not rounded) / nframes as
 * for forward(), and
 *   mels_dev     [B, Fmax, mel_dim] fp32, 16-byte aligned: the TARGET mels; frame f is fed mels[f - 1] (a zero frame first: gta.py:34-36 happens inside)
 *   keep_dev     [B, Fmax, 2, prenet_dim] bytes, 4-byte aligned: the prenet's keep masks as for forward(), or NULL for no dropout
 *   zone_dev     [B, Fmax, 4, decoder_dim] bytes: zoneout (model.py:154-166 — on with is_training=False too), 1 = keep the PREVIOUS state, in the
 *                order layer 0 h, layer 0 c, layer 1 h, layer 1 c; or NULL for no zoneout.  The decoder's output is not zoned out, only the state.
 *   mel_dev      [B, Fmax, mel_dim] fp32: the mel with the postnet residual (the reference's second return value, what gta.py saves)
 *   mel_pre_dev  the same shape, or NULL: the mel before the postnet (the first return value)
 * Rows past nframes[b] are zero in both.  With explicit masks a row's result does not depend on the batch it is in; every sum is a fixed-order
 * chain.  The prenet, its share of the gates and the projection are GEMMs over all frames ahead of / behind the frame loop, which is two launches
 * per frame.  `lengths` follows this library's rule (tokens past a row's length do not exist); the reference's corpus run treats the padded
 * columns of a batch as tokens — pass lengths = Lmax and nframes = Fmax for every row to reproduce that.
 * fp32 products only: with the option "bf16x3" set the call returns VTTS_ERR_INVALID.  Workspace: forward_teacher_workspace_bytes().
 */
int vtts_nat_acoustic_forward_teacher_workspace_bytes(const vtts_nat_acoustic* h, int B, int Lmax, int Fmax, size_t* bytes);
int vtts_nat_acoustic_forward_teacher(vtts_nat_acoustic* h, const int32_t* tokens_dev, const int32_t* lengths_dev, const float* durations_dev,
                                      const int32_t* nframes_dev, int B, int Lmax, int Fmax, const float* mels_dev, const uint8_t* keep_dev,
                                      const uint8_t* zone_dev, float* mel_dev, float* mel_pre_dev, void* workspace, size_t workspace_bytes, void* stream);
/*
 * keep_dev and zone_dev of forward_teacher() as the REFERENCE draws them from the checkpoint's rng (model.py:149 -> :95-100, :162-165): with
 * (K_n, S_n) = jax.random.split(K_{n-1}), S_1 and S_2 are the prenet's two dropouts, each ONE draw uniform(S, (B, F, prenet_dim)) < 0.5, and
 * S_3 .. S_6 are bernoulli(S, 0.1, (B, F, decoder_dim)) for layer 0 h, layer 0 c, layer 1 h, layer 1 c.  Each draw covers the whole tensor, so a
 * row's masks depend on B, F and its row index (unlike inference, where every sentence gets the same per-frame masks).  threefry_partitionable as
 * for keep_masks_haiku_mode: 0 = jax.random's classic layout, 1 = the unpinned restatement of JAX >= 0.5's default.
 * Restatement: tests/_gta_oracle.py::haiku_teacher_masks.
 */
int vtts_nat_acoustic_teacher_masks_haiku(const vtts_nat_acoustic* h, uint32_t rng_key0, uint32_t rng_key1, int threefry_partitionable, int B, int F,
                                          uint8_t* keep_dev, uint8_t* zone_dev, void* stream);
/* Valid for the groups of the handle's LAST forward_groups() call (VTTS_ERR_STATE otherwise). */
int vtts_nat_acoustic_wait_group(vtts_nat_acoustic* h, int group, void* stream);
/*
 * The token encoder alone, then the rest from its output (the text -> waveform pipeline: the encoder needs the tokens only, so it runs while
 * the host still turns the duration model's seconds into frame counts).  enc_dev [B, Lmax, 2 * encoder_dim] fp32.  A row of it does not
 * depend on its batch: rows may be re-ordered or dropped between the two calls (B and the row order of forward_from_encoder() are its own;
 * Lmax must be encode()'s).  encode() needs workspace_bytes(h, B, Lmax, 1).  forward_from_encoder(ngroups = 0) gives forward()'s mel,
 * ngroups >= 1 forward_groups()'s hand-over: the same mel, bit for bit.
 */
int vtts_nat_acoustic_encode(vtts_nat_acoustic* h, const int32_t* tokens_dev, const int32_t* lengths_dev, int B, int Lmax, float* enc_dev,
                             void* workspace, size_t workspace_bytes, void* stream);
int vtts_nat_acoustic_forward_from_encoder(vtts_nat_acoustic* h, const float* enc_dev, const int32_t* lengths_dev, const float* durations_dev,
                                           const int32_t* nframes_dev, int B, int Lmax, int Fmax, const uint8_t* keep_dev, float* mel_dev,
                                           void* workspace, size_t workspace_bytes, void* stream, int ngroups, const int32_t* group_row0,
                                           const int32_t* group_frames);

/* ------------------------------------------------------------------------------------------------------------------
 * Streaming session: forward() cut along TIME, for a caller who wants the first audio before the last frame is decoded (the reference has
 * nothing like it: vietTTS/synthesizer.py:33-39 computes the whole mel, then the whole waveform).  The decoder runs up to a frame cursor, the
 * mel is made final (postnet + residual) for one frame window after the other, and a finished window may be vocoded while the decoder carries
 * on.  Every kernel and every sum is forward()'s: after the last window mel_dev equals forward()'s result in every byte, and after every window
 * the frames below its end already do.  One session per handle; B >= 1 rows, all starting at frame 0.
 *
 * The postnet is 5 x Conv1D(k = 5): a frame of its output reads 5 * (5 - 1) / 2 = 10 frames of the decoder's mel on either side, so a window
 * [f0, f1) is computed on a copy of the frames [max(0, f0 - 10), min(Fmax, f1 + 10)) in a compact buffer (the convolutions bound and zero-fill
 * their stores by the row pitch, so they are not pointed into the full rows) and only [f0, f1) is copied out.  (fp64, 75 frames: the window's
 * interior equals the whole-row postnet to 1.3e-15 with 10 halo frames, and differs by 2.7e-2 with 9.)
 *
 *   stream_workspace_bytes()  workspace_bytes(h, B, Lmax, Fmax) plus the compact window buffers; max_window = the largest f1 - f0 of a finish().
 *   stream_begin()    forward()'s arguments and checks (and mel_dev 16-byte aligned).  Enqueues the token encoder and the conditioning gates of
 *                     ALL frames on `stream` — a session puts nothing on the handle's side stream, so no later call has an event to wait for —
 *                     and zeroes the decoder's state and mel_dev (rows past nframes[b] are zero as after forward()).  The arrays must stay
 *                     allocated and unchanged until the session ends.  The frame loop of a session is the per-frame launches: the option
 *                     "resident" is ignored ("resident_used" reads 0), "stage_times" records nothing, "bf16x3" is honoured as set at begin()
 *                     (changing it inside a session makes decode() / finish() return VTTS_ERR_STATE).  A stream that is being captured is
 *                     refused with VTTS_ERR_INVALID.
 *   stream_decode()   enqueues the decoder's frames [cursor, min(upto, Fmax)) and moves the cursor; upto <= cursor does nothing (VTTS_OK).
 *   stream_finish()   mel_dev[b][f0 .. f1) = postnet + residual, for every row.  Windows come in order and contiguous: the first f0 is 0, every
 *                     later f0 the previous f1, f1 > f0 (an f1 past Fmax counts as Fmax) and f1 - f0 <= max_window, else VTTS_ERR_INVALID; the
 *                     cursor must have reached min(f1 + VTTS_NAT_POSTNET_HALO, Fmax), else VTTS_ERR_STATE.  A refused call enqueues nothing.
 *   stream_end()      forgets the session (nothing is enqueued; frames not decoded stay undecoded).  forward*(), encode() and stream_begin() on
 *                     the handle end an open session too.  decode() / finish() without a session return VTTS_ERR_STATE.
 * The calls of a session are ordered by the stream(s) they are given: use one stream, or order them yourself.
 */
#define VTTS_NAT_POSTNET_HALO 10
int vtts_nat_acoustic_stream_workspace_bytes(const vtts_nat_acoustic* h, int B, int Lmax, int Fmax, int max_window, size_t* bytes);
int vtts_nat_acoustic_stream_begin(vtts_nat_acoustic* h, const int32_t* tokens_dev, const int32_t* lengths_dev, const float* durations_dev,
                                   const int32_t* nframes_dev, int B, int Lmax, int Fmax, const uint8_t* keep_dev, float* mel_dev, void* workspace,
                                   size_t workspace_bytes, int max_window, void* stream);
int vtts_nat_acoustic_stream_decode(vtts_nat_acoustic* h, int upto, void* stream);
int vtts_nat_acoustic_stream_finish(vtts_nat_acoustic* h, int f0, int f1, void* stream);
int vtts_nat_acoustic_stream_end(vtts_nat_acoustic* h);

/* ------------------------------------------------------------------------------------------------------------------
 * Slot pool: the streaming session with a frame cursor PER ROW, for a caller who serves many sentences that do not start together (continuous
 * batching; the reference has nothing like it).  A frame step costs about the same for 1 row as for 32, so the rows a lone sentence leaves idle
 * are capacity: a sentence joins the running batch at any tick, in a free slot, and leaves when it is done, while its neighbours carry on.
 * A TICK is one frame step of every slot: the session's three launches per frame, row b at frame tick - start[b] (start[] on the device, written
 * by admit()), idle while that is negative or >= its frame count.  The state ping-pong goes by the tick's parity.  Every output element depends
 * on its own sentence's column only, and every sum is forward()'s chain: a row's decoder mel and, after its windows, its mel equal forward()'s of
 * that sentence alone in every byte, whatever its slot, its start tick and its neighbours.
 *
 *   pool_workspace_bytes()  stream_workspace_bytes(h, slots, Lmax, Fmax, max_window) plus the per-slot words.
 *   pool_open()     keep_dev [slots, Fmax, 2, prenet_dim] bytes or NULL (no dropout), mel_dev [slots, Fmax, mel_dim] fp32, 16-byte aligned; both and the
 *                   workspace stay allocated until the pool ends.  Zeroes the state, mel_dev and the slots' words on `stream`; every slot is free.  Ends an
 *                   open session.  The option "resident" is ignored ("resident_used" reads 0), "bf16x3" is honoured as set at open() (changing it
 *                   makes every later pool call return VTTS_ERR_STATE).
 *   pool_admit()    a sentence into a free slot: tokens_dev [Lmax] (`length` of them real) and durations_dev [Lmax] (FRAMES, fp32) must stay allocated
 *                   until the slot is retired; nframes in 1 .. Fmax.  The caller fills the slot's rows of keep_dev first, in stream order.  Enqueues on
 *                   `stream`, behind the ticks enqueued so far: the slot's reset (its columns of both state parities and of the cell states, its rows
 *                   of the decoder's mel and of mel_dev zero; start, frame and token counts set), then the token encoder and the conditioning gates of
 *                   all of the row's frames, as a one-row call on the slot's rows of the workspace.  The next tick decodes the row's frame 0.
 *   pool_decode()   enqueues `nticks` ticks for all slots (nticks = 0 does nothing).  The host keeps every slot's start tick, frame count and finished
 *                   frame; a row's cursor is clamp(tick - start, 0, nframes).
 *   pool_finish()   mel_dev[slot][f0 .. f1) = postnet + residual for each of the n listed rows (HOST arrays; a slot at most once), all in ONE postnet pass
 *                   over compact windows.  Per row stream_finish()'s rules: the first f0 is 0, every later f0 the row's previous f1, f1 > f0 (an f1 past
 *                   the row's frames counts as its frame count), f1 - f0 <= max_window, else VTTS_ERR_INVALID; the row's cursor must have reached
 *                   min(f1 + VTTS_NAT_POSTNET_HALO, nframes), else VTTS_ERR_STATE.  Rows not listed are untouched.  No host synchronisation.
 *   pool_retire()   frees a busy slot, finished or not: behind the ticks enqueued so far its row decodes no further frame.  Its rows of mel_dev stay
 *                   as they are until the slot is admitted again.
 *   pool_close()    forgets the pool (nothing is enqueued).  forward*(), encode() and stream_begin() on the handle end an open pool too: a handle has
 *                   a pool or a session, never both.
 * VTTS_ERR_INVALID: a slot out of range, length > Lmax, nframes outside 1 .. Fmax, a stream that is being captured.  VTTS_ERR_STATE: admit() into a busy
 * slot, retire() or finish() on a free one, any of open's successors without an open pool, the option "bf16x3" changed since open().  A refused
 * call enqueues nothing.  The calls of a pool are ordered by the stream(s) they are given: use one stream, or order them yourself.
 */
int vtts_nat_acoustic_pool_workspace_bytes(const vtts_nat_acoustic* h, int slots, int Lmax, int Fmax, int max_window, size_t* bytes);
int vtts_nat_acoustic_pool_open(vtts_nat_acoustic* h, int slots, int Lmax, int Fmax, int max_window, const uint8_t* keep_dev, float* mel_dev, void* workspace,
                                size_t workspace_bytes, void* stream);
int vtts_nat_acoustic_pool_admit(vtts_nat_acoustic* h, int slot, const int32_t* tokens_dev, int length, const float* durations_dev, int nframes, void* stream);
int vtts_nat_acoustic_pool_decode(vtts_nat_acoustic* h, int nticks, void* stream);
int vtts_nat_acoustic_pool_finish(vtts_nat_acoustic* h, int n, const int32_t* slots, const int32_t* f0, const int32_t* f1, void* stream);
int vtts_nat_acoustic_pool_retire(vtts_nat_acoustic* h, int slot, void* stream);
int vtts_nat_acoustic_pool_close(vtts_nat_acoustic* h);

#ifdef __cplusplus
}
#endif
#endif /* VTTS_NAT_H */
