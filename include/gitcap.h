/*
 * gitcap.h - C ABI of libgitcap.so: MI355X (gfx950) native GIT-style video-caption inference.
 *
 * The reference (farazali7/real-time-video-captioning) has no FFI/plugin layer: its boundary is
 * duck-typed Python methods on the model object.  Each entry point below names the reference
 * call it stands behind (paths relative to the reference root), so a maintainer can bind it with
 * ctypes (gitcap/model.py is that binding).
 *
 * Conventions
 *   - every function returns 0 on success or a negative gitcap_status; the message is read with
 *     gitcap_last_error(h) (h may be NULL for errors raised by gitcap_create);
 *   - no C++ exception crosses this boundary;
 *   - the caller owns every input/output buffer (device memory unless stated otherwise);
 *     the handle owns weights, KV cache and workspace;
 *   - work is enqueued on `stream` (a hipStream_t passed as void*; NULL = default stream) and is
 *     asynchronous; nothing on the data path synchronises the device -- only the set-up and diagnosis calls do
 *     (gitcap_load_tensor / _finalize_weights, gitcap_set_compute / _set_fp8_scale, gitcap_fp8_saturations, and gitcap_poll_errors
 *     when it has a failure to report).  One data-path call waits on the host without synchronising the device:
 *     gitcap_student_greedy_draft / gitcap_student_window_greedy_draft wait for an event behind their own verify pass;
 *   - a handle is bound to one device and is not thread-safe.
 */
#ifndef GITCAP_H
#define GITCAP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gitcap gitcap_t;

typedef enum {
    GITCAP_OK = 0,
    GITCAP_ERR_ARG = -1,      /* bad argument / shape outside what the handle was created for */
    GITCAP_ERR_STATE = -2,    /* call order violated (e.g. decode before prefill, weights missing) */
    GITCAP_ERR_HIP = -3,      /* a HIP runtime call failed */
    GITCAP_ERR_NOMEM = -4,
    GITCAP_ERR_EXCHANGE = -5  /* a fused GEMM + LayerNorm launch gave up waiting for its sibling tiles (see gitcap_poll_errors) */
} gitcap_status;

typedef enum { GITCAP_F32 = 0, GITCAP_BF16 = 1 } gitcap_dtype;

/* greedy stop rules */
typedef enum {
    GITCAP_STOP_NEVER = 0,    /* always run max_len steps (fixed work; bench) */
    GITCAP_STOP_ALL_SEP = 1   /* reference rule: stop when ALL rows emit SEP in the same step
                                 (src/models/model.py:184); rows keep generating after their own SEP */
} gitcap_stop;

/* Hyper-parameters: src/models/model.py:681-718 (get_git_model) and
 * data/teacher_configs/GIT_LARGE_MSRVTT/parameter.yaml:1-3.  Field order is mirrored by
 * gitcap.config.CGitCapConfig. */
typedef struct gitcap_config {
    int32_t image_size, patch_size;
    int32_t enc_width, enc_layers, enc_heads, enc_ffn;
    int32_t dec_width, dec_layers, dec_heads, dec_ffn;
    int32_t vocab_size, max_text_pos;
    int32_t num_frames;            /* num_image_with_embedding; 0 = no temporal embedding */
    int32_t cls_token_id, sep_token_id, pad_token_id;
    float enc_ln_eps, dec_ln_eps, proj_ln_eps;
    int32_t max_batch;             /* clips per call the workspace is sized for */
    int32_t max_frames;            /* frames per clip */
    int32_t max_text_len;          /* text positions per row (CLS + generated) */
    int32_t max_beams;             /* >= 1 */
} gitcap_config;

/* Replaces: get_git_model(tokenizer, param)            src/models/model.py:681-718
 *           GenerativeImageTextTeacher.__init__          src/models/model.py:726-745 */
int gitcap_create(const gitcap_config* cfg, int device, gitcap_t** out);
void gitcap_destroy(gitcap_t* h);
const char* gitcap_last_error(const gitcap_t* h);

/* Replaces: load_state_dict(self.model, ckpt)            src/models/model.py:736-738
 * `name` is a canonical tensor name (gitcap/weights.py); `data` is HOST memory, fp32, row-major.
 * The library converts GEMM weights to bf16 (round-to-nearest-even) and keeps tables, biases and
 * LayerNorm parameters in fp32.  gitcap_finalize_weights fails if any tensor is missing. */
int gitcap_load_tensor(gitcap_t* h, const char* name, const float* data,
                       const int64_t* shape, int rank);
int gitcap_finalize_weights(gitcap_t* h);

/* Storage of the GEMM weights in HBM (BASELINE.json configs[4]: "GIT-large fp8 weights"; the reference's teacher is
 * data/teacher_configs/GIT_LARGE_MSRVTT/parameter.yaml:1-3).  Call before the first gitcap_load_tensor.
 * GITCAP_W_FP8_E4M3: every GEMM weight is kept as OCP e4m3 bytes + one power-of-two fp32 scale per output row, half
 * the bytes of bf16.  The values passed to gitcap_load_tensor must already be e4m3 x 2^k (weight-only quantisation is
 * the caller's choice: gitcap.weights.quantize_weights_fp8); anything else is refused, nothing is rounded silently.
 * The weight-streaming text kernels read the e4m3 bytes and expand them in registers (times the row scale: exactly the
 * bf16 value); the big-tile GEMMs of the image pass read each panel through a bf16 staging buffer.  Arithmetic is unchanged (bf16 MFMA, fp32 accumulate): results
 * are bitwise those of bf16 storage of the same values.  Under bf16 compute this is a CAPACITY option (half the weight bytes in
 * HBM), not a speed option: the staging launches cost 0.25 ms per BASELINE configs[4] batch (14.1 vs 13.8 ms; pipelined 353 vs 358
 * captions/s) and the token loop's saving on the weight stream does not make that up at 4 clips x 4 beams; it pays together with
 * GITCAP_COMPUTE_FP8_FFN below (12.8 ms; pipelined 398 captions/s), whose GEMMs read the codes as stored. */
typedef enum { GITCAP_W_BF16 = 0, GITCAP_W_FP8_E4M3 = 1 } gitcap_weight_storage;
int gitcap_set_weight_storage(gitcap_t* h, int storage);
/* device bytes of all loaded tensors (weights, scales, tables, biases) */
/* Arithmetic of the image pass (north_star: "MFMA bf16/fp8 GEMMs"; BASELINE configs[4]).  GITCAP_COMPUTE_BF16 (default): every GEMM
 * on bf16 operands.  GITCAP_COMPUTE_FP8_FFN (opt-in; needs e4m3 weight storage and 768- / 1024-wide models): FC1 and FC2 of the
 * image rows run on v_mfma_f32_16x16x128_f8f6f4 with the e4m3 weight codes read as stored and activations quantised to e4m3 with a
 * static scale (default: codes of value * 16, saturating at +-28; gitcap_set_fp8_scale / gitcap_fp8_saturations below) by the
 * producing epilogues; everything else stays bf16.  Results differ from
 * bf16 compute by the activation rounding (measured |dlogit| <= 0.3 of a spread of 4 on GIT-large: docs/LAB_NOTEBOOK.md par. 3 / 6); the oracle's
 * counterpart is GitOracle(emulate_fp8_act="ffn"). */
enum { GITCAP_COMPUTE_BF16 = 0, GITCAP_COMPUTE_FP8_FFN = 1 };
int gitcap_set_compute(gitcap_t* h, int compute);
/* The static scale of the e4m3 activation codes of GITCAP_COMPUTE_FP8_FFN (no reference counterpart: the reference computes in
 * fp32, src/models/model.py:378, :412-418).  A code holds value / scale; codes reach +-448, so the default 1/16 covers +-28 and
 * e.g. 1/4 covers +-112 at four times the rounding step.  `scale` must be a power of two in [2^-16, 2^8].  The mode saturates,
 * but never silently: every code of a valid row that the producing epilogues clamp at +-448 is counted on the device, and
 * gitcap_fp8_saturations reads (and, with reset != 0, clears) the count since the last reset.  Both calls synchronise the
 * device.  A caller calibrates by running representative clips and raising the scale until the count stays 0; the oracle's
 * counterpart is GitOracle(emulate_fp8_act="ffn", fp8_scale=...). */
int gitcap_set_fp8_scale(gitcap_t* h, float scale);
int gitcap_fp8_saturations(gitcap_t* h, int64_t* count, int reset);
int gitcap_weight_bytes(const gitcap_t* h, int64_t* bytes);

/* Format of the image-prefix V rows the TOKEN LOOP reads (north_star: "a KV cache for the decode loop ... bf16/fp8"; the reference
 * has no cache at all, src/models/model.py:412-418 recomputes the prefix for every token).  GITCAP_KV_BF16 (default): the q|k|v
 * GEMM output of the decoder's image rows as it is.  GITCAP_KV_V_E4M3 (opt-in): a second copy of the V rows as OCP e4m3 codes with
 * one power-of-two scale per (token, head), written once per clip behind each decoder layer's q|k|v GEMM; the text rows' attention
 * reads K in bf16 and V from the codes (3/4 of the bytes of its K/V stream).  K stays bf16 in every mode: a peaked head's scores do
 * not survive a 6 % step on a key (profiles/r05_fp8_kv_cache_study.txt: up to 2.5 on logits of std 4).  The image rows' own
 * attention, the text rows' own K/V and all arithmetic are unchanged; results differ from the default by the rounding of V
 * (measured |dlogit| 0.10 plain / 0.5 stress weights); the oracle's counterpart is GitOracle(emulate_fp8_v=True).  The exact
 * KV-cache property (cached step == teacher-forced pass, bitwise) and batch invariance hold in either mode.  Synchronises the device;
 * +3/8 of the image K/V bytes of workspace (4 slots). */
enum { GITCAP_KV_BF16 = 0, GITCAP_KV_V_E4M3 = 1 };
int gitcap_set_kv_cache(gitcap_t* h, int mode);

/* Replaces: self.image_encoder(torch.stack(batch['image'])) + temporal add + cat(dim=1)
 *                                                         src/models/model.py:378-382
 *           the 'linearLn' visual projection              src/models/model.py:699
 *           and the image half of self.textual(...)       src/models/model.py:412-418
 * frames: device [B,F,3,H,W] fp32 NCHW (layout of src/utils/dataloader.py:60-82).
 * visual_out (nullable): device fp32 [B, F*N, enc_width] = ln_post + temporal embedding
 * (the `visual_features` the reference returns at model.py:424 / :460).
 * Because image tokens never attend to text (GIT block mask) their decoder K/V are text
 * independent: this call also runs the projected image tokens through the decoder layers and
 * leaves their K/V in the handle (the exact KV cache every later text call reads). */
int gitcap_encode(gitcap_t* h, const float* frames, int B, int F, float* visual_out, void* stream);

/* Same as the second half of gitcap_encode, starting from caller-supplied visual features
 * (device fp32 [B, S_img, enc_width]); lets forward_decoder(y, memory) honour `memory`. */
int gitcap_set_visual(gitcap_t* h, const float* visual, int B, int S_img, void* stream);

/* Replaces: self.textual(visual_features, caption_tokens)  src/models/model.py:412-418
 *           scores = step(input_ids)                        src/models/model.py:519
 * Runs text positions t0 .. t0+T-1 of `rows` rows through the decoder against the cached image
 * K/V of clip (row / beams) and the row's own cached text K/V (text->image full, text->text
 * causal), appending their K/V to the text cache.  Positions < t0 must have been run before.
 * ids: device int64, token of row r / position t0+j at ids[r*ld_ids + j].
 * logits_out (nullable): device fp32 [rows, T, vocab] when all_positions != 0 (teacher-forced
 * logits of forward_output_logits, model.py:747-760), else [rows, vocab] for position t0+T-1.
 * argmax_out (nullable): device int64, argmax of the last position's logits written to
 * argmax_out[r*ld_argmax]. */
int gitcap_text_forward(gitcap_t* h, const int64_t* ids, int ld_ids, int rows, int beams,
                        int t0, int T, float* logits_out, int all_positions,
                        int64_t* argmax_out, int ld_argmax, void* stream);

/* Replaces: the third return of GenerativeImageTextModel.forward_one_custom (hidden_states, stacked per layer)
 *                                                         src/models/model.py:419-424, :747-760
 * Opt-in (it costs a copy of every row after every layer, and the image rows of the LAST decoder layer, which are
 * otherwise never computed: only their K/V are needed).  While enabled, gitcap_encode / gitcap_set_visual and a
 * gitcap_text_forward with t0 = 0 keep the decoder stack's input and the output of each of its layers;
 * gitcap_hidden_states_read writes them as out[b][e][s][:], device fp32 [B][dec_layers + 1][S_img + T][dec_width]
 * (e = 0: projected image tokens ; text embeddings, e = l: output of layer l; s over [image ; text]).
 * Synchronous entry points only (not the pipelined submissions). */
int gitcap_hidden_states_enable(gitcap_t* h, int enable);
int gitcap_hidden_states_read(gitcap_t* h, int B, int S_img, int T, float* out, void* stream);

/* Replaces: StudentCandidateV1.greedy_decode(src, max_len) src/models/model.py:156-187
 *           as called by src/real_time_inference.py:58 and src/inference.py:51
 * Encodes, prefills with CLS and runs max_len greedy steps entirely on the device.
 * ids_out: device int64 [B, max_len+1] (column 0 = CLS).  steps_out: device int32[1] = number
 * of generated columns that are valid under `stop` (the host truncates to 1+steps). */
int gitcap_greedy(gitcap_t* h, const float* frames, int B, int F, int max_len, int stop,
                  int64_t* ids_out, int32_t* steps_out, void* stream);

/* Replaces: image_transform()                          src/utils/dataloader.py:18-32
 *                                                         src/real_time_inference.py:16-28
 * ToTensor -> Resize(crop, bicubic, tensor path) -> CenterCrop(crop) -> BGR->RGB -> Normalize(CLIP),
 * applied on the device to nf raw frames: frames_hwc_bgr device uint8 [nf][H][W][3] (OpenCV layout,
 * real_time_inference.py:39) -> out_nchw device fp32 [nf][3][crop][crop], the layout gitcap_encode reads.
 * Stateless (no handle). */
int gitcap_preprocess(const uint8_t* frames_hwc_bgr, int nf, int H, int W, float* out_nchw, int crop, void* stream);

/* The two calls above for RAW camera frames (what src/real_time_inference.py:39-57 has before its transform):
 * frames_hwc_bgr device uint8 [B][F][H][W][3].  The transform of gitcap_preprocess (crop = image_size) is fused with
 * the patch gather of the encoder (SURVEY.md par. 8f.1): the bf16 patch rows are written directly, no fp32 frame tensor
 * exists.  Results are bitwise those of gitcap_preprocess followed by gitcap_encode / gitcap_greedy. */
int gitcap_encode_raw(gitcap_t* h, const uint8_t* frames_hwc_bgr, int B, int F, int H, int W, float* visual_out, void* stream);
int gitcap_greedy_raw(gitcap_t* h, const uint8_t* frames_hwc_bgr, int B, int F, int H, int W, int max_len, int stop,
                      int64_t* ids_out, int32_t* steps_out, void* stream);

/* Replaces: F.log_softmax(scores) + beam_scores, view(B, beams*V), torch.topk(2*beams)
 *                                                         src/models/model.py:557-565
 * logits: device fp32 [B*beams][ld]; beam_scores: device fp32 [B*beams]; outputs: device
 * out_scores fp32 [B][K], out_idx int32 [B][K] (flat index beam*V + word), sorted descending,
 * ties by smaller flat index; K <= 16, beams <= 16, V <= 131072 (else GITCAP_ERR_ARG, nothing is launched).  Logits of -inf are
 * no candidates; if a clip has fewer than K candidates its remaining slots hold score -inf, index 0x7fffffff.  Stateless (no handle). */
int gitcap_beam_topk(const float* logits, int ld, const float* beam_scores, int B, int beams, int V, int K,
                     float* out_scores, int32_t* out_idx, void* stream);

/* Replaces: GenerativeImageTextModel.infer + GeneratorWithBeamSearchV2.search
 *                                                         src/models/model.py:426-462, :479-678
 * (do_sample = False; num_keep_best = 1 and no repetition penalty, the way GenerativeImageTextTeacher.forward drives it, :768,
 * unless gitcap_attach_search_options says otherwise for this call).
 * The whole search runs on the device with no host round trip: per step decoder forward, beam top-k
 * (log-softmax + beam scores, :557-565), hypothesis/beam bookkeeping (:573-621) and the KV reorder the
 * reference leaves commented out (:623-634).  decoded_out: device int64 [B][max_steps], CLS-prefixed best
 * hypothesis padded with EOS (:671-675); logprobs_out: device fp32 [B] (:665).  The reference's early
 * `break` when every sentence is done (:640) is not needed for correctness (done sentences ignore their
 * candidates) and is not taken: all max_steps-1 steps are enqueued. */
int gitcap_beam_search(gitcap_t* h, const float* frames, int B, int F, int beams, int max_steps,
                       float length_penalty, int per_node_beam_size,
                       int64_t* decoded_out, float* logprobs_out, void* stream);

/* Pipelined form of gitcap_greedy for a stream of batches (no reference counterpart: the reference
 * processes one clip at a time, src/models/model.py:765).  submit enqueues the image pass on the
 * handle's encoder stream and the text loop on one of its two decoder streams, ordered after the work already
 * on `stream` (so `frames` may be produced there), and returns a ticket; at most FOUR submissions
 * may be in flight (four slots), so one batch's MFMA-bound image pass overlaps the latency-bound
 * token loops of the batches before it.  wait makes `stream` wait for that submission's ids_out/steps_out.
 * frames / ids_out / steps_out must stay valid until the wait. */
int gitcap_greedy_submit(gitcap_t* h, const float* frames, int B, int F, int max_len, int stop,
                         int64_t* ids_out, int32_t* steps_out, void* stream, int* ticket);
int gitcap_greedy_wait(gitcap_t* h, int ticket, void* stream);

/* The same pipelined form for gitcap_beam_search (BASELINE configs[4]; the reference's teacher runs this search one clip at a time,
 * src/models/model.py:762-768 with the defaults of :702-708): the image pass of one batch overlaps the search loops of the batches
 * before it.  Tickets of both submit forms share one sequence (at most FOUR submissions of either kind in flight);
 * gitcap_beam_search_wait is gitcap_greedy_wait under the name that pairs with this call.  visual_out (nullable): as in gitcap_encode
 * (the `visual_features` of the reference's output dict, model.py:460).  step_logits_out (nullable): device fp32
 * [max_steps - 1][B * beams][vocab], the raw logits of every search step (what model.py:521 appends to saved_logits).
 * Results are bitwise those of gitcap_beam_search. */
int gitcap_beam_search_submit(gitcap_t* h, const float* frames, int B, int F, float* visual_out, int beams, int max_steps,
                              float length_penalty, int per_node_beam_size,
                              int64_t* decoded_out, float* logprobs_out, float* step_logits_out, void* stream, int* ticket);
int gitcap_beam_search_wait(gitcap_t* h, int ticket, void* stream);

/* The two pipelined submissions for RAW camera frames in device memory (frames_hwc_bgr device uint8 [B][F][H][W][3], as in
 * gitcap_greedy_raw): the transform of src/utils/dataloader.py:18-32 / src/real_time_inference.py:16-28 fused with the patch
 * gather runs as the first launch of the image pass on the handle's encoder stream.  This is the form a HOST-fed caller uses
 * (src/real_time_inference.py:39-58 holds OpenCV frames in host memory; src/inference.py:45-51 a DataLoader's CPU tensor): the
 * caller enqueues the copy of batch i + 1 (a quarter of the bytes of the fp32 tensor) on the stream it passes as `stream`, so the
 * copy runs under batch i's compute and only the image pass waits for it (gitcap/model.py: _StagingRing is that caller; keep to
 * the caller's own stream -- with a fifth stream the runtime's four hardware queues are oversubscribed and a copy queues behind
 * a token loop: measured 1 618 against 2 004 captions/s, profiles/r06_host_fed_copy_stream.txt).  Results are bitwise those of gitcap_greedy_raw / of gitcap_preprocess +
 * gitcap_beam_search.  Tickets, slots and waits as for gitcap_greedy_submit. */
int gitcap_greedy_raw_submit(gitcap_t* h, const uint8_t* frames_hwc_bgr, int B, int F, int H, int W, int max_len, int stop,
                             int64_t* ids_out, int32_t* steps_out, void* stream, int* ticket);
int gitcap_beam_search_raw_submit(gitcap_t* h, const uint8_t* frames_hwc_bgr, int B, int F, int H, int W, float* visual_out,
                                  int beams, int max_steps, float length_penalty, int per_node_beam_size,
                                  int64_t* decoded_out, float* logprobs_out, float* step_logits_out, void* stream, int* ticket);

/* Sliding frame window for live captioning (the reference's loop, src/real_time_inference.py:44-57, collects six sampled frames,
 * captions them and clears its list: one caption per six new frames, each re-encoding frames it has never seen).  A caption of the
 * last F frames after every new one would encode each frame F times through gitcap_greedy.  The ViT encodes every frame on its own,
 * and the temporal embedding is added after ln_post: so the handle keeps a ring of the fp32 ln_post rows (embedding NOT added) of
 * the last F frames of B clips that advance in lockstep, a push encodes only the new frames, and a window call adds each frame's
 * embedding at its current position and runs the decoder's image prefix (which does depend on the whole window) and the token loop.
 *
 * gitcap_window_reset: B = 0 releases the ring.  Otherwise (re)allocates it for B <= max_batch clips and F <= max_frames (and
 * <= num_frames when num_frames > 0) frames, and empties it.  Set-up call: may synchronise.
 * gitcap_window_push: encode n (1 <= n <= F) new frames per clip and append them to the ring.  frames: device [B][n][3][S][S] fp32
 * (as gitcap_encode); gitcap_window_push_raw: raw uint8 BGR [B][n][H][W][3] (as gitcap_encode_raw).  Frame j of a push is older
 * than frame j + 1.
 * gitcap_window_greedy / _beam_search: caption the current window (the last F frames pushed, oldest = temporal embedding 0);
 * outputs as gitcap_greedy / gitcap_beam_search, visual_out (nullable, 16-byte aligned) as gitcap_encode's.
 *
 * Results: window_greedy's ids and steps are bitwise those of gitcap_greedy on the window's F frames, in the same weight-storage,
 * compute and KV-cache mode; visual_out is bitwise gitcap_encode's; window_beam_search is bitwise gitcap_beam_search; the _raw push
 * is bitwise gitcap_preprocess followed by gitcap_window_push.
 * Isolation: a push writes only encoder workspace and the ring -- not slot 0's image K/V, the text cache or the current image, so a
 * gitcap_text_forward after a push continues against the previous image.  A window call leaves slot 0 exactly as gitcap_greedy
 * would.  Other synchronous calls and pipelined submissions made between pushes do not disturb the ring; pushes order themselves
 * behind submissions in flight like every other synchronous entry point.  Pushes and window calls may be issued on different
 * streams: each push waits for an event recorded behind the last window call's image prefix, each window call for one recorded
 * behind the last ring write (no device synchronisation).
 * Errors: GITCAP_ERR_ARG when B differs from the reset's, n < 1, n > F, or a pointer is null or misaligned; GITCAP_ERR_STATE for a
 * push before any reset and a window call before F frames have been pushed since the reset; GITCAP_ERR_EXCHANGE (gitcap_poll_errors
 * semantics): the ring's rows are undefined, so the window is emptied (as after a reset) and the error is returned once -- push the
 * last F frames again.
 * Workspace: gitcap_workspace_bytes counts the ring while it is allocated, B * F * N * enc_width * 4 bytes (58 MB at 16 clips x 6
 * frames of GIT-base); the push stages its rows in the image pass's own q|k|v buffer.  A handle that never resets a window
 * allocates nothing. */
int gitcap_window_reset(gitcap_t* h, int B, int F);
int gitcap_window_push(gitcap_t* h, const float* frames, int B, int n, void* stream);
int gitcap_window_push_raw(gitcap_t* h, const uint8_t* frames_hwc_bgr, int B, int n, int H, int W, void* stream);
int gitcap_window_greedy(gitcap_t* h, int max_len, int stop, float* visual_out,
                         int64_t* ids_out, int32_t* steps_out, void* stream);
int gitcap_window_beam_search(gitcap_t* h, int beams, int max_steps, float length_penalty, int per_node_beam_size,
                              float* visual_out, int64_t* decoded_out, float* logprobs_out, void* stream);

/* Stream pool: the frame window for several cameras on one handle.  The window above is ONE ring cursor: its B clips receive the same
 * n frames per push and no caption comes before all of them hold F frames.  Cameras behind scene-change gates of their own admit
 * frames at different times: each is at its own fill level and ring position.  The pool keeps n_streams independent windows
 * (streams) of F frames over a ring of the same rows (fp32 ln_post, temporal embedding NOT added), takes frames for any of them in
 * any mix -- every frame is encoded once -- and captions any subset of them as one ragged batch.
 * Contract: row r of gitcap_pool_greedy / gitcap_pool_beam_search is bit for bit row r of gitcap_greedy / gitcap_beam_search with
 * the streams' frame counts attached (gitcap_attach_frame_counts) on the streams' current frames, oldest first, and so, as there,
 * what the stream's frames give alone: ids, log-probabilities, alternatives, scores.  When every named stream holds the same
 * number of frames the layout is the dense one and the call takes the dense launches, as equal attached counts do.
 *   reset   1 <= n_streams <= 4096 with a ring of n_streams * F * tokens_per_frame * enc_width * 4 bytes <= 8 GiB (3.6 MB per stream
 *           at F = 6 on GIT-base); 1 <= F <= max_frames, F <= 255 (and <= num_frames when num_frames > 0).  Allocates the ring and
 *           three int32 tables of max_batch * max_frames entries (or, for the sizes of the last reset, reuses them) and empties every
 *           stream.  n_streams = 0 releases all of it.  A set-up step: a change of sizes waits for the device.  The pool is state of
 *           its own: gitcap_window_* neither read nor change it, nor the pool calls the window; a handle that never resets a pool
 *           allocates nothing and runs exactly the launches it ran before.
 *   push    frames: device fp32 [n][3][S][S], 16-byte aligned (_raw: uint8 BGR [n][H][W][3]); stream_ids: HOST int32 [n]: frame i
 *           goes to stream stream_ids[i] behind that stream's earlier frames, this push's earlier ones included.  1 <= n <=
 *           max_batch * max_frames, and a stream gets at most F frames in one push (more would write one ring frame twice in one
 *           launch: push twice).  The ids are checked on the host before anything is enqueued; a refused push changes nothing.
 *           Work: the encoder pass of n one-frame clips (the ragged path's, without the temporal add) and one scatter launch.  Like
 *           a window push it writes neither slot 0's image K/V nor the text cache.
 *   greedy / beam_search   stream_ids: HOST int32 [B], 1 <= B <= min(max_batch, 256), distinct; decoder row r is stream
 *           stream_ids[r], in the caller's order, and sees its last n_r = min(frames pushed, F) frames; the named streams hold at
 *           most max_batch * max_frames frames together.  frames_out (host int32 [B], nullable) = n_r.  The other arguments and the
 *           outputs as gitcap_window_greedy / gitcap_window_beam_search without visual_out.  Work: one assemble launch (each frame's
 *           temporal embedding at its position in its OWN clip), the image prefix, the token loop.  Attachments: what the window
 *           calls take (token log-probabilities, top-k alternatives, prompt, constraints; search options and sampling); attached
 *           frame counts are refused (and consumed) with the window calls' message.  There is no draft form, no visual_out, no
 *           attention map and no _submit form of the pool calls.
 *   drop    empties one stream (a camera that reconnected); the others are untouched.
 *   counts  host int32 [n_streams]: the frames each stream holds, 0 .. F.
 * Pushes and pool calls may be issued on different streams (two events order a push behind the last pool call's image prefix and
 * the last push, and a pool call behind the last push); pushes of the pool and of the window, which share the encoder workspace,
 * wait for each other's events too.  The two page-locked tables are reused behind an event each.
 * Errors: GITCAP_ERR_ARG for a null handle or pointer, misaligned frames, sizes outside the bounds above, a stream id outside
 * [0, n_streams), more than F frames for one stream in one push, a stream named twice in a call, attached frame counts, and the
 * checks of gitcap_greedy / gitcap_beam_search; GITCAP_ERR_STATE for a call before any reset (or after the release), a named stream
 * that holds no frame (nothing is launched) and weights not finalized; GITCAP_ERR_EXCHANGE as for the window: every stream is
 * emptied and the error is returned once -- push again.  Workspace: gitcap_workspace_bytes counts the ring and the tables while they
 * are allocated.  gitcap_abi_version is unchanged: these are new symbols only. */
int gitcap_pool_reset(gitcap_t* h, int n_streams, int F);
int gitcap_pool_push(gitcap_t* h, const float* frames, const int32_t* stream_ids, int n, void* stream);
int gitcap_pool_push_raw(gitcap_t* h, const uint8_t* frames_hwc_bgr, const int32_t* stream_ids, int n, int H, int W, void* stream);
int gitcap_pool_greedy(gitcap_t* h, const int32_t* stream_ids, int B, int max_len, int stop, int64_t* ids_out, int32_t* steps_out,
                       int32_t* frames_out, void* stream);
int gitcap_pool_beam_search(gitcap_t* h, const int32_t* stream_ids, int B, int beams, int max_steps, float length_penalty,
                            int per_node_beam_size, int64_t* decoded_out, float* logprobs_out, void* stream);
int gitcap_pool_drop(gitcap_t* h, int stream_id);
int gitcap_pool_counts(const gitcap_t* h, int32_t* counts_out);

/* Greedy decoding that verifies a draft caption in one pass, accepted row by row (the teacher's counterpart of
 * gitcap_student_greedy_draft; the reference has none).  gitcap_greedy_draft = gitcap_greedy, gitcap_window_greedy_draft =
 * gitcap_window_greedy: *steps_out, ids_out[b][0 .. *steps_out] and the attached log-probabilities of those steps are bit for bit
 * those of the call without a draft, whatever the draft holds (with GITCAP_STOP_NEVER that is every column).  A cached token step
 * equals the teacher-forced position bit for bit, so ONE pass over the draft's n_draft positions yields the token the loop would
 * emit behind every draft prefix.  Each clip keeps its OWN leading matches plus the loop's token at its first mismatch (covered_b
 * = min(a_b + 1, n_draft) steps); the token loop resumes at the first step some clip lacks (min_b covered_b), clips ahead of it keep
 * the tokens they hold; it is skipped when nothing is left or all rows emitted SEP in a step every clip covers (GITCAP_STOP_ALL_SEP).
 *   draft_ids     device int64 [B][ld_draft]: column 0 is ignored and taken as CLS, columns 1..n_draft are the guessed tokens,
 *                 1 <= n_draft <= max_len, ld_draft >= n_draft + 1; any ids (an id outside [0, vocab) can only be rejected)
 *   accepted_out  HOST int32 [B] (nullable): a_b, the leading draft tokens accepted for clip b
 * Synchronous only: the call waits on the host once, for an event behind its verify pass (not for the tail).  Takes
 * gitcap_attach_token_logprobs and (gitcap_greedy_draft) gitcap_attach_frame_counts; a pending prompt or pending constraints are
 * consumed and the call fails with GITCAP_ERR_ARG.  n_draft > 63, or B * n_draft beyond the slot's text-row workspace: the call
 * runs the plain loop, reports 0 accepted and counts as a call with nothing offered.
 * Errors: GITCAP_ERR_ARG for a null handle, draft_ids or ids_out, n_draft < 1, n_draft > max_len, ld_draft < n_draft + 1, and
 * the checks of gitcap_greedy / gitcap_window_greedy.
 * gitcap_draft_stats: host int64[4] = draft calls, draft tokens offered (n_draft per clip, summed), tokens accepted (summed over
 * the clips), tail steps run behind verify passes. */
int gitcap_greedy_draft(gitcap_t* h, const float* frames, int B, int F, const int64_t* draft_ids, int ld_draft, int n_draft, int max_len,
                        int stop, int64_t* ids_out, int32_t* steps_out, int32_t* accepted_out, void* stream);
int gitcap_window_greedy_draft(gitcap_t* h, const int64_t* draft_ids, int ld_draft, int n_draft, int max_len, int stop, float* visual_out,
                               int64_t* ids_out, int32_t* steps_out, int32_t* accepted_out, void* stream);
int gitcap_draft_stats(const gitcap_t* h, int64_t* out4);

/* Per-token log-probabilities of a greedy caption (no reference counterpart: the reference's greedy loop returns ids only).
 * A ONE-SHOT attachment: it applies to the NEXT greedy-family call or submission on the handle -- gitcap_greedy, gitcap_greedy_raw,
 * gitcap_greedy_submit, gitcap_greedy_raw_submit, gitcap_window_greedy -- and is consumed by it, whether that call succeeds or
 * fails; any other entry point (encode, text_forward, beam search, pushes) leaves a pending attachment alone; logprobs_out == NULL
 * detaches.  A pipelined submission captures the pointer: the buffer stays valid until the wait, like ids_out.
 *   logprobs_out  device fp32 [B][ld], ld >= max_len of the consuming call: column t = log_softmax(logits of step t)[ids_out[b][t + 1]],
 *                 the natural-log probability of the token the loop emitted at step t.  Columns < *steps_out are defined, later
 *                 ones unspecified; columns >= max_len are not written.
 * The values come out of the launches that choose the token (the vocabulary head leaves a third partial per 16-column tile, the
 * sum of exp(logit - tile max); the arg-max launch merges them in a fixed order): no logits tensor, no extra launch, no host round
 * trip, and bitwise independent of the batch size and of the entry point.  With or without an attachment every id is the same.
 * Errors: GITCAP_ERR_ARG for ld < 1 or a pointer that is not 4-byte aligned; at the consuming call ld < max_len gives
 * GITCAP_ERR_ARG with nothing launched (the attachment is consumed all the same).
 * Memory: the first attach on a handle allocates the third partial beside the arg-max partials, one buffer per pipeline slot (a
 * set-up step: it may synchronise; gitcap_workspace_bytes counts it from then on).  A handle that never attaches allocates
 * nothing and runs exactly the launches it ran before. */
int gitcap_attach_token_logprobs(gitcap_t* h, float* logprobs_out, int ld);

/* Top-k token alternatives per position (the `top_logprobs=k` of text-generation interfaces), without a logits tensor.  A ONE-SHOT
 * attachment like gitcap_attach_token_logprobs: taken, and consumed whether the call succeeds or fails, by the next of gitcap_greedy,
 * gitcap_greedy_raw, gitcap_greedy_submit, gitcap_greedy_raw_submit, gitcap_window_greedy and gitcap_score; k == 0 or a NULL pointer
 * detaches.  The beam-search family leaves it pending.  gitcap_greedy_draft and gitcap_window_greedy_draft refuse it: the call
 * consumes the attachment, launches nothing and returns GITCAP_ERR_ARG with a message that names it.
 *   top_ids  device int64 [B][ld][k], top_lp device fp32 [B][ld][k], 1 <= k <= 32, ld >= max_len of a greedy call (ld >= T - 1 of
 *            gitcap_score).  Entry [b][t][j] = the j-th best column of the distribution step t chose ids_out[b][t + 1] from, and its
 *            natural-log probability; gitcap_score: position j of row r goes to [r][j][.] for j < T - 1, counted or not, like top1_ids.
 *            Positions >= max_len (T - 1) are not written; positions >= *steps_out are unspecified.
 * Order and ties: columns are ranked by (logit descending, column ascending), the arg-max launch's tie rule: rank 0 is the token
 * the loop emitted (gitcap_score: top1_ids) and top_lp[..][0] compares == to its token log-probability (top1_lp).
 * Padding: a rank the row cannot fill -- fewer than k columns with a logit above -inf (bans, a masked bias), or vocab_size < k --
 *            holds id -1 and lp -inf.  NaN never appears for logits that are finite or -inf.
 * With a prompt attached a forced position still reports the model's own ranks (and the prompt runs as forced steps); with
 * constraints attached the step's banned columns never appear and the probabilities are those of the renormalised row; it
 * combines with the frame-count and token log-probability attachments.  With or without it every id is the same.
 * How: the head runs its three-partial form; a tile's arg-max partial is its best column, so the k best columns of a row lie in
 * its k best tiles; one workgroup per row recomputes those k x 16 logits with the head's own MFMA chain (bit for bit the head's
 * logits) and ranks them.  A row's values do not depend on the batch size or the entry point.
 * Errors: GITCAP_ERR_ARG for k outside [1, 32], ld < 1, misaligned pointers; at the consuming call ld below the positions it
 * writes gives GITCAP_ERR_ARG with nothing launched.  Memory: the first attach allocates the third partial per pipeline slot, as
 * gitcap_attach_token_logprobs does, and nothing else; a handle that never attaches runs exactly the launches it ran before. */
int gitcap_attach_top_logprobs(gitcap_t* h, int k, int64_t* top_ids, float* top_lp, int ld);
/* debug hook (no handle): the three-partial head over X [M][ldx] (bf16) against W [ceil(V / 16) * 16][D] (bf16, or e4m3 codes with
 * wscale; Wpk nullable: the fragment-major copy of gitcap_dbg_pack_frags), under ban_mask (nullable, uint16 [M][ld_mask]), then
 * the k best columns of every row -> top_ids int64 / top_lp fp32 [M][k] as described above. */
int gitcap_dbg_head_topk(const void* X, int ldx, int M, const void* W, const void* Wpk, const float* wscale, const float* bias, int V, int D,
                         int k, const uint16_t* ban_mask, int ld_mask, int64_t* top_ids, float* top_lp, void* stream);

/* Score GIVEN captions: the log-probability of every token of captions somebody else supplied (a ground truth, an n-best entry, a
 * sampled or carried caption), teacher-forced in one pass, without a logits tensor.
 *   ids   device int64 [rows][ld_ids], CLS first, T >= 2 columns used, ld_ids >= T; rows = B * beams, row r belongs to clip
 *         r / beams (the rows of a clip share its image K/V, as in gitcap_text_forward);
 *   lp[r][j] = log_softmax(logits[r][j][:])[ids[r][j + 1]],  j = 0 .. T - 2  (natural log).
 * Ignored positions: (r, j) is ignored when its target ids[r][j + 1] lies outside [0, vocab_size), when it equals ignore_id (-1:
 * none), or when lengths (nullable, device int32 [rows]: valid tokens of the row, CLS included) is given and j + 1 >= lengths[r].
 * An ignored position gets lp = 0 and is not counted.  The kernels decide this themselves: the ids live on the device.
 * -inf: a target whose logit is -inf (a masked bias column) gives lp = -inf, a row of logits that are all -inf gives -inf; for
 * logits that are finite or -inf NaN never appears.
 * Outputs (device, each nullable):
 *   token_lp  fp32 [rows][ld_lp], ld_lp >= T - 1; columns >= T - 1 are not written;
 *   row_sum   fp32 [rows]: the counted positions' lp added in ascending position order by one thread (one fixed order);
 *   row_cnt   int32 [rows]: the number of counted positions;
 *   top1_ids  int64 / top1_lp fp32 [rows][T - 1]: the model's own arg-max at each position (ignored ones included) and its
 *             log-probability, under the tie rule and bit for bit the values of the greedy loop's arg-max launch
 *             (gitcap_dbg_argmax_final_lp on the same partials).
 * How: the vocabulary head runs in a form of its own that stores no logits and leaves, beside the three per-tile partials of the
 * token log-probabilities, the one logit of each row's given next token; one workgroup per (row, position) merges the partials in
 * the fixed order of the greedy loop and forms (y_t - M) - log(total); a second small launch adds the rows.  Every element comes
 * from the same MFMA chain and the same merge order whatever else is in the call: a row's values are bit for bit independent of
 * the other rows, of `beams` and of the form of the head kernel.
 * Preconditions and argument checks are gitcap_text_forward's with t0 = 0 (after gitcap_encode / gitcap_set_visual; rows ==
 * encoded clips * beams; rows <= max_batch * max_beams; T <= max_text_len), plus GITCAP_ERR_ARG for T < 2, ld_ids < T or
 * ld_lp < T - 1; a refused call launches nothing.  Synchronous path, slot 0: it overwrites the text K/V of positions 0..T-1.
 * Memory: the first call allocates the third partial (as gitcap_attach_token_logprobs does) and 8 bytes per text row of the slot;
 * gitcap_workspace_bytes counts them from then on.  A handle that never scores runs exactly the launches it ran before. */
int gitcap_score(gitcap_t* h, const int64_t* ids, int ld_ids, int rows, int beams, int T, const int32_t* lengths, int64_t ignore_id,
                 float* token_lp, int ld_lp, float* row_sum, int32_t* row_cnt, int64_t* top1_ids, float* top1_lp, void* stream);
/* debug read: the first n target logits the last gitcap_score captured (head row m = r * T + j; rows without a target in range
 * keep whatever they held) -> out (device fp32 [n]) */
int gitcap_dbg_score_target_logits(gitcap_t* h, float* out, int n, void* stream);

/* Per-token attention maps over frames and patches: which image tokens every position of a caption attends to, read back from the
 * q | k the LAST SYNCHRONOUS text pass of the handle left in its text cache (gitcap_greedy and its raw / window / draft forms,
 * gitcap_score, gitcap_distill, gitcap_text_forward from position 0 and the calls that extended it).  Nothing is recomputed and no
 * existing launch changes: two small launches over the cache.
 * For row r (clip r / rows-per-clip of that pass), position j, decoder layer l and head h, p[l][h][r][j][.] is the softmax of
 * q . k / sqrt(64) over the clip's image keys followed by the row's text keys 0 .. j (the mask the decoder applies).  The outputs are
 * means over the heads and over the selected layers, layer = -1: all, layer = l: that one:
 *   frame_mass  device fp32 [rows][T][ld_f]: column f = the mass on the image tokens of frame f of the row's clip (its class token
 *               included); columns from the clip's frame count to the longest clip's hold 0; ld_f >= frames of the longest clip
 *   text_mass   device fp32 [rows][T]: the mass on the row's own text keys; frame_mass summed over f + text_mass = 1 up to rounding
 *   patch_map   nullable, device fp32 [rows][T][ld_s]: column s = the mean probability of image token s of the clip (frame-major),
 *               0 from the clip's token count to the longest clip's; ld_s >= image tokens of the longest clip
 *   lengths     nullable, device int32 [rows]: positions j >= lengths[r] are written as zeros
 * Columns beyond the widths named above are not written.  Position j is the one whose head predicts token j + 1.  Sums run in a
 * fixed order without float atomics: a row's values do not depend on the rows beside it and repeat bit for bit.
 * Errors: GITCAP_ERR_STATE when there is no such pass (none yet, an image pass or a submitted call since), when the last pass was a
 * beam search or gitcap_reorder_rows moved the rows (their rows are permuted: score the predictions, then ask), when T exceeds the
 * positions that pass filled, or when the image prefix is not whole frames; GITCAP_ERR_ARG for rows != that pass's rows, a layer
 * outside [-1, dec_layers), short leading dimensions, null outputs.  The first call allocates the scratch (2 floats per layer,
 * head, row and position of the handle's sizes). */
int gitcap_attention_map(gitcap_t* h, int rows, int T, int layer, const int32_t* lengths, float* frame_mass, int ld_f, float* text_mass,
                         float* patch_map, int ld_s, void* stream);
/* The same two launches on caller-built caches, no handle: kv_txt bf16 [L][rows][Tmax][3 D] (q | k | v of the text rows), kv_img bf16
 * [L][img_rows][3 D]; clip c's image keys are rows c * S_img .. of kv_img (off == len == NULL, Smax == S_img), or rows off[c] ..
 * off[c] + len[c] - 1 (device int32 [rows / rows_per_clip], len[c] a multiple of N and <= Smax).  N = image tokens per frame,
 * D == 64 H.  The scratch is a stream-ordered allocation.  GITCAP_ERR_ARG for what would index outside a buffer. */
typedef struct gitcap_dbg_attn_map_args {
    const void *kv_txt, *kv_img;
    int32_t L, H, D, rows, rows_per_clip, T, Tmax, N, S_img, Smax, img_rows;
    const int32_t *off, *len;
    int32_t layer;
    const int32_t* lengths;
    float* frame_mass;
    int32_t ld_f;
    float *text_mass, *patch_map;
    int32_t ld_s;
} gitcap_dbg_attn_map_args;
int gitcap_dbg_attn_map(const gitcap_dbg_attn_map_args* a, void* stream);

/* Prompted decoding: per-clip text prefixes for the greedy and the beam family -- the `prefix` branch of the reference's
 * GenerativeImageTextModel.infer (src/models/model.py:432-437, :453-455: the search starts from the given tokens instead of a lone
 * CLS; how a GIT model is asked a question, told how a caption begins, or made to continue one).  The reference takes one prefix
 * (`assert len(batch['prefix']) == 1`); here every clip has its own, of its own length.
 * A ONE-SHOT attachment with the life cycle of gitcap_attach_token_logprobs / gitcap_attach_search_options / gitcap_attach_sampling
 * and combinable with all three: it applies to the NEXT call or submission of the greedy family (gitcap_greedy, gitcap_greedy_raw,
 * their _submit forms, gitcap_window_greedy) or of the beam family (gitcap_beam_search, its _submit / _raw_submit forms,
 * gitcap_window_beam_search), whichever comes first, and is consumed by it whether that call succeeds or is refused; every other
 * entry point leaves it pending; prompt_ids == NULL and lengths == NULL detach.  A pipelined submission captures the two pointers:
 * the buffers stay valid and unchanged until the wait.  The student model takes its prompts through an attachment of its own
 * (gitcap_student_attach_prompt).
 *   prompt_ids  device int64 [B][ld], CLS at column 0 (the beam family starts every row from the handle's CLS whatever column 0 says).
 *   lengths     device int32 [B]: valid tokens per clip, CLS included, 1 <= lengths[b] <= ld; 1 = no prompt for that clip.
 *   min_len, max_len  the host's minimum and maximum of lengths (launches are planned without a round trip).  The kernels clamp
 *               lengths[b] to [1, max_len], so a mismatch reads nothing outside the clip's row.
 * Ids outside the vocabulary are the caller's error: they are written to the output as given, and the text embedding clamps them
 * into its table (< 0 -> row 0, >= vocab_size -> the last row), as it does for every id gitcap_text_forward is handed.
 * Greedy: ids_out[b][0 .. lengths[b] - 1] is the prompt, the columns behind it are the model's; a step that writes a position
 * inside a row's prompt takes the prompt's token instead of the arg-max, for the output and for the next step's input alike.  A
 * forced token is not counted by the stop rule (GITCAP_STOP_ALL_SEP looks at what the model emitted), and an attached
 * log-probability buffer gets 0.0f at a forced position, as gitcap_score gives an ignored one (gitcap_score supplies the values of
 * given tokens).  Positions 0 .. min_len - 1 run as ONE multi-position pass where the slot's row workspace holds B * min_len rows
 * (always on the synchronous path): a P-token prompt shared by all rows costs one pass, not P token steps.  Because a cached token
 * step is bit for bit the teacher-forced position, the ids do not depend on that plan, on the batch, or on the other rows' lengths.
 * Beam: as the reference, the prompt is the start of input_ids, the beam scores start at [0, -1e9, ..] and prompt tokens add
 * nothing to a score; max_steps counts the prompt and so does the length penalty's cur_len (:592-594); the repetition penalty sees
 * the prompt's tokens.  A clip at cur_len < lengths[b] is forced: it is not ranked, every beam appends prompt_ids[b][cur_len],
 * src_rows is the identity, and beam_scores, done and the hypothesis slots are untouched.  decoded_out / the n-best include the prompt.
 * Errors: GITCAP_ERR_ARG for one null pointer, a misaligned pointer, or min_len < 1, max_len < min_len, ld < max_len; at the
 * consuming call max_len > the call's max_len (greedy) or > max_steps - 1 (beam) gives GITCAP_ERR_ARG with nothing launched (the
 * attachment is consumed all the same).  A handle that never attaches runs exactly the launches it ran before. */
int gitcap_attach_prompt(gitcap_t* h, const int64_t* prompt_ids, int ld, const int32_t* lengths, int min_len, int max_len);

/* Per-clip frame counts: a batch whose clips differ in length, packed -- no padding, no masking.
 *   counts   HOST int32 [B] (copied by the call): clip b has counts[b] frames, 1 <= counts[b] <= min(max_frames, num_frames when
 *            the model has temporal embeddings, 255); B <= min(max_batch, 256).
 * A ONE-SHOT attachment with the life cycle of gitcap_attach_prompt: the next call of gitcap_encode, gitcap_encode_raw, the greedy
 * family or the beam family (their _submit / _raw_submit forms included) consumes it, whether that call succeeds or is refused;
 * NULL detaches.  In the consuming call `frames` holds the sum(counts) frames clip-major (clip b's frames adjacent), B is the
 * attachment's B and F the largest count; visual_out receives the packed rows [sum(counts) * N][enc_width].  It combines with the
 * log-probability, prompt, constraint, search-option and sampling attachments.
 * Layout: clip b's image rows -- encoder output, decoder input, the per-layer image K/V and the opt-in e4m3 V codes and scales --
 * start at off[b] = N * sum_{i<b} counts[i] and number len[b] = N * counts[b]; off / len live in the pipeline slot as device
 * int32 arrays.  Every GEMM sees the N * sum(counts) valid rows; the decoder's image-prefix attention and the text rows' attention
 * run their variable-length forms; the temporal embedding is added by a row kernel from a per-frame position table (the fp32 add
 * of the fused epilogue).  A clip inside a ragged batch is bit for bit the clip captioned alone.  Later calls that read the
 * slot's image prefix (gitcap_text_forward, gitcap_score, gitcap_distill, gitcap_reorder_rows, the token loops) follow the slot's
 * tables.  Equal counts take the dense path, launch for launch.
 * Errors, all GITCAP_ERR_ARG with a last_error text: a count of 0 or above the limit, B outside its range, a sum beyond
 * max_batch * max_frames (at the attach); B or F that disagree with the counts (at the consuming call); gitcap_set_visual and the
 * window family (gitcap_window_reset / _push / _push_raw / _greedy / _beam_search) with counts attached (the attachment is
 * consumed); gitcap_hidden_states_read while slot 0 holds a ragged prefix. */
int gitcap_attach_frame_counts(gitcap_t* h, const int32_t* counts, int B);

/* Constrained decoding: hard limits on what a step may emit.  Before a step ranks, arg-maxes or samples row r, every banned column
 * of that row is -inf, and everything downstream sees the banned row: the head's tile partials, the chunk statistics, the
 * log-softmax, the top-k / top-p filter, the token log-probabilities.  The edit sits where the reference edits its logits
 * (src/models/model.py:522-531, ahead of the log_softmax at :557), so the probabilities renormalise over the allowed columns -- a
 * deliberate difference from HF's beam search, which masks after normalising.  With prefix = the row's ids so far (CLS and any prompt
 * included) and cur_len its length, the banned set of a row is the union of
 *   no_repeat_ngram_size = n >= 1 (HF NoRepeatNGramLogitsProcessor): prefix[i + n - 1] for every i in 0 .. cur_len - n with
 *       prefix[i .. i + n - 2] == prefix[cur_len - n + 1 .. cur_len - 1]; nothing while cur_len + 1 < n; n = 1: every token of the
 *       prefix.  Ids are compared as values; an id outside [0, vocab_size) bans nothing.
 *   min_length = m (HF MinLengthLogitsProcessor): the model's SEP while cur_len < m; m counts CLS and the prompt.
 *   suppress (HF SuppressTokensLogitsProcessor): up to 256 ids banned at every step; duplicates allowed, ids outside the
 *       vocabulary ignored.
 * A position forced by a prompt (gitcap_attach_prompt) takes the prompt's token whatever is banned; under a repetition penalty -inf
 * stays -inf.  gitcap_score, gitcap_distill and gitcap_text_forward are not constrained; the student model takes the same rules
 * through an attachment of its own (gitcap_student_attach_constraints).
 * A ONE-SHOT attachment with the life cycle of gitcap_attach_prompt: the next call of the greedy family (gitcap_greedy,
 * gitcap_greedy_raw, their _submit forms, gitcap_window_greedy) or of the beam family (gitcap_beam_search, its _submit / _raw_submit
 * forms, gitcap_window_beam_search, sampled or not) consumes it, whichever comes first, whether that call succeeds or is refused;
 * every other entry point leaves it pending; NULL detaches.  It combines with the log-probability, search-option, sampling and
 * prompt attachments.  A pipelined submission captures `suppress`: the buffer stays valid and unchanged until the wait.
 * Each step of a constrained call makes one more small launch (the rows' ban mask, uint16 [rows][ld_mask], bit c & 15 of word
 * c >> 4 = column c, built from the buffer that holds each row's current prefix; in the beam family the rows are the B * beams
 * beam rows) and runs the BAN form of the vocabulary head (greedy) or of the candidate ranking / sampling kernel (beam).  The mask
 * buffers -- one per pipeline slot, max_batch * max_beams rows -- are allocated by the first attach (a set-up step that may
 * synchronise; gitcap_workspace_bytes counts them from then on); a handle that never attaches allocates nothing and runs exactly
 * the launches it ran before.  A prompted greedy call with constraints attached runs its prompt as forced token steps: the one-pass
 * plan of gitcap_attach_prompt is not combined with constraints (same ids either way).
 * Errors, all GITCAP_ERR_ARG: a negative field; n_suppress > 256; n_suppress > 0 with a null or misaligned pointer; a vocabulary
 * above 131072 columns; at the consuming call n_suppress + max_len >= vocab_size (greedy) or n_suppress + max_steps + beams *
 * per_node_beam_size > vocab_size (beam): a row could otherwise lose every column, or a clip be left with fewer candidates than
 * the bookkeeping ranks.  Nothing is launched then and the attachment is consumed all the same. */
typedef struct gitcap_constraints {
    int32_t no_repeat_ngram_size;   /* 0 = off, else 1..max_text_len */
    int32_t min_length;             /* 0 = off; counts CLS and the prompt */
    const int32_t* suppress;        /* device int32 [n_suppress], nullable when n_suppress == 0 */
    int32_t n_suppress;             /* 0..256 */
} gitcap_constraints;
int gitcap_attach_constraints(gitcap_t* h, const gitcap_constraints* c);   /* NULL detaches */

/* The kernels behind it, one launcher each on caller-owned device buffers (tests/test_constraints_gpu.py).
 * gitcap_dbg_ban_mask: one workgroup per row writes every word of mask_out [rows][ld_mask] (ld_mask even, >= ceil(V / 16); the
 * result does not depend on what the buffer held) from prefix_ids int64 [rows][ld_ids] (columns 0 .. cur_len - 1) and the device
 * list suppress int32 [n_suppress]; V <= 131072.
 * gitcap_dbg_vocab_head_banned: gitcap_dbg_vocab_head_lse under mask uint16 [M][ld_mask]; amax_sum NULL selects the plain form.
 * gitcap_beam_topk_constrained / gitcap_sample_rows_constrained: gitcap_beam_topk_penalized / gitcap_sample_rows under mask
 * [B * beams][ld_mask]; repetition_penalty = 1 selects the unpenalised BAN form.  Each equals its unconstrained call on logits
 * that hold -inf at the banned columns, bit for bit. */
int gitcap_dbg_ban_mask(const int64_t* prefix_ids, int ld_ids, int rows, int cur_len, int n, int min_length, int sep_id,
                        const int32_t* suppress, int n_suppress, int V, uint16_t* mask_out, int ld_mask, void* stream);
/* gitcap_dbg_ban_mask with its rules read on the device when the kernel runs (tests/test_student_constraints_gpu.py): rec, device
 * int32 [4 + 256] = {n, min_length, n_suppress, 0, the suppress ids}; n_suppress is clamped on the device to 0..256.  Same mask. */
int gitcap_dbg_ban_mask_rec(const int64_t* prefix_ids, int ld_ids, int rows, int cur_len, int sep_id, const int32_t* rec, int V,
                            uint16_t* mask_out, int ld_mask, void* stream);
int gitcap_dbg_vocab_head_banned(const void* X, int ldx, const void* W, const float* wscale, const float* bias, int M, int N, int K,
                                 float* logits, float* amax_val, int32_t* amax_idx, float* amax_sum, const uint16_t* mask, int ld_mask,
                                 void* stream);
int gitcap_beam_topk_constrained(const float* logits, int ld, const float* beam_scores, const int64_t* prefix_ids, int ld_ids, int cur_len,
                                 float repetition_penalty, int B, int beams, int V, int K, float* out_scores, int32_t* out_idx,
                                 const uint16_t* mask, int ld_mask, void* stream);
int gitcap_sample_rows_constrained(const float* logits, int ld, const float* beam_scores, const int64_t* prefix_ids, int ld_ids, int cur_len,
                                   float repetition_penalty, int B, int beams, int V, int per_node, float temperature, int top_k, float top_p,
                                   uint64_t seed, float* out_scores, int32_t* out_idx, int32_t* kept_out, float* logz_out,
                                   const uint16_t* mask, int ld_mask, void* stream);

/* Options of the device-resident search: the reference's search operator keeps `num_keep_best` finished hypotheses per clip and
 * applies a `repetition_penalty` (GeneratorWithBeamSearchV2.search, src/models/model.py:479-678; the penalty :522-531, the n-best
 * output :653-678).  A ONE-SHOT attachment, like gitcap_attach_token_logprobs: it applies to the NEXT beam-family call or
 * submission on the handle -- gitcap_beam_search, gitcap_beam_search_submit, gitcap_beam_search_raw_submit,
 * gitcap_window_beam_search -- and is consumed by it, whether that call succeeds or fails; every other entry point (encode,
 * text_forward, the greedy family, pushes, waits) leaves a pending attachment alone; opt == NULL detaches.  A pipelined submission
 * captures the two pointers: the buffers stay valid until the wait, like decoded_out.
 *   repetition_penalty  before the candidates of a step are ranked, every logit whose column occurs in the row's prefix (CLS
 *                       included) becomes x < 0 ? x * rp : x / rp -- once however often the token occurs, -inf stays -inf, plain fp32
 *                       IEEE multiply / divide -- and the log-softmax is taken over the penalised row.  step_logits_out stays raw
 *                       (model.py:521 saves before :522).  1.0: no penalty, the ranking launches are those without options.
 *   num_keep_best = n   BeamHypotheses with n slots: while fewer than n hypotheses are stored a finished one is stored; afterwards it
 *                       replaces the stored minimum (the earliest stored among equal minima) only if its score is strictly greater;
 *                       a clip is done once n are stored and the minimum >= best candidate sum / (max_steps - 1)^length_penalty.
 *   nbest_out           device int64 [B][n][max_steps]: the stored hypotheses by descending score (equal scores in storage order),
 *                       CLS first, EOS padded; a rank with no hypothesis is all-EOS.
 *   nbest_logprobs_out  device fp32 [B][n]: their scores; -1e5 for a rank with no hypothesis (model.py:654).
 * The call's own decoded_out / logprobs_out receive rank 0 of the n-best under the attached options.  With n > 1 the done rule
 * waits for n hypotheses and compares against the WORST of them, so a clip searches on where n = 1 would have stopped: rank 0 need
 * not equal the result of the same call without options.  With n = 1 both pointers may be NULL; if given they receive a copy.
 * Errors: GITCAP_ERR_ARG for num_keep_best outside [1, 16], a penalty that is not finite and > 0, a missing pointer with n > 1, a
 * pointer that is not aligned to its element; at the consuming call n > beams * per_node_beam_size gives GITCAP_ERR_ARG with
 * nothing launched (the attachment is consumed all the same).
 * Memory: the first attach with n > 1 allocates the n-best state, once per pipeline slot, sized for max_batch clips x 16
 * hypotheses x (max_text_len + 1) ids (a set-up step: it may synchronise; gitcap_workspace_bytes counts it from then on).  A handle
 * that never attaches allocates nothing and runs exactly the launches it ran before. */
typedef struct gitcap_search_options {
    int32_t num_keep_best;       /* 1..16; at the consuming call also <= beams * per_node_beam_size */
    float   repetition_penalty;  /* finite, > 0; 1.0 = none */
    int64_t* nbest_out;          /* device int64 [B][num_keep_best][max_steps]; required when num_keep_best > 1, else nullable */
    float*   nbest_logprobs_out; /* device fp32 [B][num_keep_best]; same rule */
} gitcap_search_options;
int gitcap_attach_search_options(gitcap_t* h, const gitcap_search_options* opt);

/* gitcap_beam_topk under a repetition penalty: prefix_ids device int64 [B*beams][ld_ids], the first cur_len columns of row r are
 * the tokens whose logits in row r are penalised (ids outside [0, V) are ignored; see gitcap_search_options for the rule).  Same
 * limits, outputs and refusals as gitcap_beam_topk; also GITCAP_ERR_ARG for a penalty that is not finite and > 0 and, unless the
 * penalty is 1.0 (then the call IS gitcap_beam_topk and prefix_ids is not read), for a null or misaligned prefix_ids, cur_len < 1
 * or ld_ids < cur_len.  Stateless (no handle). */
int gitcap_beam_topk_penalized(const float* logits, int ld, const float* beam_scores, const int64_t* prefix_ids, int ld_ids,
                               int cur_len, float repetition_penalty, int B, int beams, int V, int K,
                               float* out_scores, int32_t* out_idx, void* stream);

/* Sampling on the device: the do_sample branch of the reference's search operator (model.py:532-554: temperature,
 * top_k_top_p_filtering with min_tokens_to_keep = 2, per_node_beam_size draws per beam row) in place of the K best candidates.  A
 * ONE-SHOT attachment with the life cycle of gitcap_attach_search_options: consumed by the NEXT beam-family call whether it succeeds
 * or is refused; it combines with a pending gitcap_attach_search_options (n-best, penalty; either may come first); opt == NULL detaches.
 * The draw is a contract of this library (torch.multinomial's stream cannot be reproduced):
 *   random numbers  Philox4x32-10, key = (seed low word, seed high word), counter = (v / 4, row, cur_len, 0) for column v of row
 *                   row = b * beams + j at step cur_len; output lane v % 4 is column v's; u = ((x >> 8) + 0.5) * 2^-24, strictly inside
 *                   (0, 1).  No state, no host round trip: a caption depends on (seed, the clip's position in the batch, logits) only,
 *                   not on the entry point or the pipeline slot.  A clip's draws DO depend on its position in the batch.
 *   the row         raw logits, penalised at the prefix columns (gitcap_search_options), divided by temperature when it is not 1,
 *                   filtered, log-softmax of the filtered row.
 *   the filter      top_k > 0: k' = min(max(top_k, 2), V), every column below the k'-th largest value is dropped, ties with it stay.
 *                   top_p < 1, on the softmax of the top-k-filtered row: column v stays iff fewer than 3 columns are strictly greater
 *                   or the probability mass of the strictly greater columns is <= top_p (ranks 0, 1, 2 of the reference's sort stay
 *                   unconditionally).  Columns of equal value share one fate: the reference's choice among equal values is the order
 *                   its sort happens to leave them in, which is no contract.  -inf columns are never kept.
 *   the draw        the per_node_beam_size largest of key_v = z_v - log(-log u_v) over the kept columns (z: the filtered row), in
 *                   descending key order, ties to the smaller column: sampling without replacement, the distribution of
 *                   torch.multinomial(softmax(z), replacement=False).  score = log_softmax(z)[word] + beam_score[row].
 *   candidates      clip b has K = beams * per_node_beam_size, UNSORTED: candidate p is draw p % per_node_beam_size of row
 *                   b * beams + p / per_node_beam_size with flat index (p % beams) * V + word (model.py:549-552 tiles the beam offsets
 *                   over the row; kept as written).  The bookkeeping takes the maximum of the K scores for the done test, walks the
 *                   candidates as given and pads only the missing beams of a clip left with fewer than `beams` live ones.
 * The same inputs give the same bits run to run (every sum has a fixed order).  step_logits_out stays the raw logits.
 * Errors: GITCAP_ERR_ARG for a temperature that is not finite and > 0, top_k < 0, top_p outside (0, 1]; at the consuming call for a
 * per_node_beam_size greater than the columns the filter is sure to keep -- per_node_beam_size > 2 with top_p < 1, or
 * 0 < max(top_k, 2) < per_node_beam_size -- or on a handle whose vocabulary is wider than 32768 columns (the kernel holds a row in
 * LDS), with nothing launched (the attachment is consumed all the same).
 * Preconditions: a row offers at least per_node_beam_size finite logits (a row that runs out of kept columns yields sentinel
 * candidates, which the bookkeeping passes over: the clip then continues with fewer live beams, padded as above).
 * Memory: none.  A handle that never attaches runs exactly the launches it ran before. */
typedef struct gitcap_sampling_options {
    float    temperature;   /* finite, > 0 */
    int32_t  top_k;         /* >= 0; 0 = off */
    float    top_p;         /* (0, 1]; 1 = off */
    uint64_t seed;
} gitcap_sampling_options;
int gitcap_attach_sampling(gitcap_t* h, const gitcap_sampling_options* opt);

/* The stateless row call behind it, beside gitcap_beam_topk / gitcap_beam_topk_penalized: logits device fp32 [B*beams][ld], prefix_ids
 * as gitcap_beam_topk_penalized (read only when repetition_penalty != 1), out_scores fp32 / out_idx int32 [B][beams * per_node] in
 * the candidate layout above; kept_out (nullable) int32 [B*beams]: the columns the filter kept; logz_out (nullable) fp32 [B*beams]:
 * the log-sum-exp of the filtered row.  A row with fewer than per_node kept columns fills the rest with (-inf, 0x7fffffff).
 * GITCAP_ERR_ARG as gitcap_beam_topk (beams > 16, beams * per_node > 16, per_node > V, ld < V), for V > 32768 (the row is held in
 * the CU's LDS) and for the values gitcap_attach_sampling refuses. */
int gitcap_sample_rows(const float* logits, int ld, const float* beam_scores, const int64_t* prefix_ids, int ld_ids, int cur_len,
                       float repetition_penalty, int B, int beams, int V, int per_node, float temperature, int32_t top_k, float top_p,
                       uint64_t seed, float* out_scores, int32_t* out_idx, int32_t* kept_out, float* logz_out, void* stream);

/* Host-side staging copy for host-fed callers (no reference counterpart): bytes from pageable memory (a DataLoader batch without
 * pin_memory, OpenCV frames) into a page-locked staging buffer, split over up to 8 threads -- as many as the process may really use
 * (affinity mask, cgroup CPU quota; GITCAP_HOST_COPY_THREADS overrides).  Plain memcpy semantics, blocking, no device work.
 * (A framework's own parallel copy may size its pool to the whole machine: under a CPU quota that costs tens of milliseconds per
 * 58 MB batch, measured; this is the copy gitcap/model.py: _StagingRing uses.) */
int gitcap_host_copy(void* dst, const void* src, int64_t bytes);

/* Health of the in-kernel statistics exchange (no reference counterpart).  The residual GEMMs that normalise their own output
 * rows exchange LayerNorm statistics between the workgroups of a row block (co-residency).  If a workgroup ever
 * gives up waiting (about 30 s: its siblings cannot become resident because another process or a CU-masked stream holds the
 * CUs) the kernel does NOT trap: it raises a host-visible flag and finishes with undefined rows.  Every entry point above
 * checks the flag first and gitcap_poll_errors checks it on demand (call it after synchronising the stream to vouch for the
 * results just produced).  Once raised: the device is drained, the flag is cleared, the handle switches for good to the
 * unfused GEMM + LayerNorm launches (bitwise the same results) and GITCAP_ERR_EXCHANGE is returned ONCE -- the caller
 * re-runs the calls whose results it had not yet vouched for.  Submissions (gitcap_greedy_submit / gitcap_beam_search_submit)
 * that were in flight at that moment are marked: their gitcap_*_wait returns GITCAP_ERR_EXCHANGE every time it is called, so a
 * retry cannot hand out their undefined ids; they must be submitted again.  Returns 0 when healthy. */
int gitcap_poll_errors(gitcap_t* h);

/* Beam reorder of the text part of the KV cache (what src/models/model.py:623-634 sketches):
 * new row r takes the cached text K/V of old row src_rows[r]; image K/V are shared. */
int gitcap_reorder_rows(gitcap_t* h, const int32_t* src_rows, int rows, int t_len, void* stream);
/* Instrumentation used by bench.py (no reference counterpart: the reference has no profiler,
 * SURVEY.md par. 5).  When enabled every launch of a kernel class is bracketed by two HIP events
 * recorded on the launch stream; gitcap_profile_read waits for them, sums the elapsed times and
 * the algorithmic flops/bytes of the bracketed launches, and resets the class. */
enum {
    GITCAP_PROF_GEMM = 0,       /* bf16 MFMA GEMM (patch-embed, qkv, proj, fc1, fc2, vproj) */
    GITCAP_PROF_ATTN_FULL = 1,  /* flash attention over frames / image prefix */
    GITCAP_PROF_SKINNY = 2,     /* text-row weight-streaming GEMMs (incl. vocabulary head) and their reduce+LayerNorm */
    GITCAP_PROF_ATTN_TEXT = 3,  /* text-row attention over the KV cache */
    GITCAP_PROF_ROWOPS = 4,     /* LayerNorm over the image rows (launches of its own) */
    GITCAP_PROF_GEMM_LN = 5,    /* the residual GEMMs that also normalise their output rows (counted here, not in class 0) */
    GITCAP_PROF_CLASSES = 6
};
int gitcap_profile_enable(gitcap_t* h, int enable);
int gitcap_profile_read(gitcap_t* h, int cls, double* ms_total, int64_t* launches,
                        double* flops_total, double* bytes_total);

/* Kernel-level test hooks (tests/test_kernels_gpu.py, tools/gemm_bench.py): run ONE kernel on
 * caller-owned device buffers.  gemm: out[m][n] = sum_k A[m][k]*W[n][k] (+epilogue `epi` of
 * csrc/kernels.h: 0 bias->bf16, 1 bias+QuickGELU->bf16, 2 bias+GELU->bf16, 3 bias+resid->f32,
 * 4 bias->f32); A [M][K] bf16, W [N][K] bf16; tile = 64, 128 or 256 (square tiles: M, N multiples of the tile). */
int gitcap_dbg_gemm(const void* A, const void* W, const float* bias, const float* resid, void* out,
                    int M, int N, int K, int epi, int tile, void* stream);
/* The fp8 tile kernel (csrc/gemm256.hip): A8 [M][K] and W8 [N][K] OCP e4m3 codes (M, N multiples of 256, K of 128), out = acc * ascale *
 * wscale[n] + bias; epi 4 -> fp32 [M][N], 0 -> bf16, 8 / 9 -> e4m3 codes of quick_gelu / erf_gelu (.) * out8_inv. */
int gitcap_dbg_gemm_f8(const void* A8, const void* W8, const float* wscale, float ascale, const float* bias, void* out,
                       int M, int N, int K, int epi, float out8_inv, void* stream);
/* GEMM + bias [+ resid] followed by LayerNorm of the output rows (N = 768 or 1024).  post = 0: out_f32 = x = A W^T + bias +
 * resid, out_bf16 = LN(x) (pre-LN block); post = 1: out_f32 = out_bf16 = LN(x), resid may be NULL (post-LN block).
 * fused = 1: inside the 256x256 kernel (the tiles of a 256-row block exchange segment statistics); fused = 0: the `tile` kernel,
 * then the row kernel.  Both produce the same bits (csrc/ln_canon.h). */
int gitcap_dbg_gemm_ln(const void* A, const void* W, const float* bias, const float* resid, const float* gamma,
                       const float* beta, float eps, float* out_f32, void* out_bf16, int M, int N, int K, int post,
                       int fused, int tile, void* stream);
/* Speed-only switches at run time (what the GITCAP_* environment variables set once per process; INTEGRATION.md par. 9), so that
 * one process can check that results do not depend on them.  key 0: GEMM + LayerNorm epilogue on/off; 1: one/two-row prologue
 * on/off; 2: 256x256-tile threshold; 3: 128x128-tile threshold; 4: retired (was: 224-row tiles for synchronous calls; accepted, no effect); 5: the greedy loop's
 * arg-max launch also embeds the next step's input rows on/off; 6: polls a fused GEMM + LayerNorm workgroup waits for its
 * siblings before it gives up (0 = default; 1 forces the fail-soft path of gitcap_poll_errors in a test); 7: the text rows'
 * FC1 -> GELU -> FC2 as one launch over hidden slices on/off; 8: fragment-major copies of the text-path weights at the next
 * gitcap_finalize_weights on/off; 9: 8-wave workgroups for text-attention launches of more (row, head) units than CUs on/off;
 * 10: the vocabulary head's four-tile workgroups that share the activation rows through LDS on/off; 11: three-wave workgroups
 * that share the slab reduce of the one/two-row prologue on/off; 20: a prompted greedy loop (gitcap_attach_prompt,
 * gitcap_student_attach_prompt) runs the positions every row's prompt covers as one multi-position pass on/off (off: as forced token steps).  Returns the previous value (< 0: bad key).  The switches are process-wide atomics: a call on another thread sees either value,
 * and either value gives the same bits. */
int gitcap_dbg_config(int key, int value);
/* attn_full: qkv [G*S][3*H*64] bf16 -> ctx [G*S][H*64] bf16 */
int gitcap_dbg_attn_full(const void* qkv, void* ctx, int G, int S, int H, void* stream);
/* attn_full, variable-length form (a ragged batch's image prefix): group g = rows off[g] .. off[g] + len[g] - 1 of the packed qkv /
 * ctx; off, len device int32 [G], len[g] >= 1 (the hook drains the stream and reads them to size the grid).  Each group's rows are
 * bit for bit gitcap_dbg_attn_full(G = 1, S = len[g]) on the group alone; no other row of ctx is written. */
int gitcap_dbg_attn_full_varlen(const void* qkv, void* ctx, int G, const int32_t* off, const int32_t* len, int H, void* stream);
/* layernorm: x fp32 [rows][D] -> out_f32 / out_bf16 (either may be NULL) */
int gitcap_dbg_layernorm(const float* x, const float* gamma, const float* beta, float eps, int rows, int D,
                         float* out_f32, void* out_bf16, void* stream);

/* Token-selection hooks (tests/test_selection_gpu.py; the restatement they are compared with is tests/selection_reference.py).
 * Each runs ONE launcher of csrc/kernels.h on caller-owned device buffers; the selection rule everywhere: the largest value,
 * the smallest index among equals.
 *
 * vocab_head: the vocabulary head of the token loops (launch_skinny, fp32-logits epilogue, identity row map).  X bf16 [M][ldx]
 * (ldx >= K, a multiple of 8); W [Npad16][K] bf16 (Npad16 = N rounded up to 16; rows n >= N are read and must not be selected),
 * or OCP e4m3 codes when wscale (fp32 [Npad16], powers of two) is non-NULL (K = 128 or 768 only); bias fp32 [N] or NULL;
 * K in {64, 128, 256, 576, 768, 1024}.  logits: fp32 [M][N] or NULL.  amax_val fp32 / amax_idx int32 [M][ntiles], ntiles = Npad16 / 16
 * (both or neither): per 16-column tile the largest logit of the row and the first column that holds it.  Honours
 * gitcap_dbg_config(10, .): the four-tile workgroups that share X through LDS (N >= 64, K <= 768) or one wave per tile; same bits. */
int gitcap_dbg_vocab_head(const void* X, int ldx, const void* W, const float* wscale, const float* bias, int M, int N, int K,
                          float* logits, float* amax_val, int32_t* amax_idx, void* stream);
/* vocab_head_lse: the same launch with the third partial of the token log-probabilities: amax_sum fp32 [M][ntiles] (required, and
 * with it amax_val / amax_idx) = the sum of exp(logit - amax_val) over the tile's valid columns, 0 for a tile whose amax_val is -inf.
 * amax_val / amax_idx are bit for bit those of gitcap_dbg_vocab_head. */
int gitcap_dbg_vocab_head_lse(const void* X, int ldx, const void* W, const float* wscale, const float* bias, int M, int N, int K,
                              float* logits, float* amax_val, int32_t* amax_idx, float* amax_sum, void* stream);
/* vocab_head_score: the _lse launch in the form gitcap_score uses: targets int64 [M] (one column per row), tgt_logit fp32 [M]: the
 * lane that holds logits[m][targets[m]] also stores it to tgt_logit[m], bit for bit the value gitcap_dbg_vocab_head writes; a
 * target outside [0, N) leaves tgt_logit[m] untouched.  The three partials are bit for bit those of gitcap_dbg_vocab_head_lse.
 * logits stays nullable (gitcap_score passes NULL).  (ignore_id and lengths are gitcap_dbg_score_final's business.) */
int gitcap_dbg_vocab_head_score(const void* X, int ldx, const void* W, const float* wscale, const float* bias, int M, int N, int K,
                                float* logits, float* amax_val, int32_t* amax_idx, float* amax_sum, const int64_t* targets, float* tgt_logit,
                                void* stream);
/* score_final: the merge of gitcap_score on caller-owned buffers.  Partials [rows * T][ntiles] and tgt_logit [rows * T] are indexed
 * by head row m = r * T + j (the rows j = T - 1 are not read); ids int64 [rows][ld_ids]; V = the vocabulary the ignore rule uses.
 * Outputs as gitcap_score's; token_lp is required here. */
int gitcap_dbg_score_final(const float* amax_val, const int32_t* amax_idx, const float* amax_sum, int ntiles, const float* tgt_logit,
                           const int64_t* ids, int ld_ids, int rows, int T, const int32_t* lengths, int64_t ignore_id, int V,
                           float* token_lp, int ld_lp, float* row_sum, int32_t* row_cnt, int64_t* top1_ids, float* top1_lp, void* stream);
/* argmax_final: out[r * ld_out] = amax_idx of the best of the ntiles partials of row r * row_stride + row_off, r < rows (a row
 * whose winner carries the empty-tile index 0x7fffffff, i.e. no logit above -inf: 0); sep_cnt (nullable): sep_cnt[step] += rows whose token is sep_id.  emb (nullable, all of
 * its fields or none): the launch goes on to write row r of xf fp32 / xb bf16 [rows][D] = LayerNorm(word[token] + pos[position])
 * (word [vocab][D], pos [>= position + 1][D], gamma / beta [D]; D a multiple of 4, <= 1024; a token outside [0, vocab) is
 * clamped into the table). */
typedef struct gitcap_dbg_next_embed {
    const float *word, *pos, *gamma, *beta;
    float eps;
    int32_t D, vocab, position;
    float* xf;
    void* xb;
} gitcap_dbg_next_embed;
int gitcap_dbg_argmax_final(const float* amax_val, const int32_t* amax_idx, int ntiles, int rows, int row_stride, int row_off,
                            int64_t* out, int ld_out, int32_t* sep_cnt, int step, int sep_id, const gitcap_dbg_next_embed* emb,
                            void* stream);
/* argmax_final_lp: the same launch, and lp_out[r * ld_lp] = -log(sum_t amax_sum[t] * exp(amax_val[t] - M)), M = the row's largest
 * partial: log_softmax(logits)[token] of the row (amax_sum fp32 [rows as amax_val][ntiles], both new arguments required).  Tiles
 * with amax_val == -inf are skipped; a row with no logit above -inf gives -inf.  Summation order: thread tid of 256 takes tiles
 * tid, tid + 256, .. ascending, a xor butterfly inside each wave, then waves 0..3 in order -- the same whatever `rows` is. */
int gitcap_dbg_argmax_final_lp(const float* amax_val, const int32_t* amax_idx, int ntiles, int rows, int row_stride, int row_off,
                               int64_t* out, int ld_out, int32_t* sep_cnt, int step, int sep_id, const gitcap_dbg_next_embed* emb,
                               const float* amax_sum, float* lp_out, int ld_lp, void* stream);
/* argmax_final_forced: the launch of a prompted greedy step that writes position p = step + 1 (gitcap_attach_prompt): prompt_ids
 * int64 [rows][ld_prompt], lengths int32 [rows] (clamped to [1, max_len]; max_len <= ld_prompt).  A row with p < lengths[r] gets
 * out = prompt_ids[r][p] -- also the token of its emb row --, adds nothing to sep_cnt and gets lp_out 0.0f; every other row is
 * gitcap_dbg_argmax_final(_lp)'s, bit for bit.  amax_sum / lp_out: both or neither.  p >= max_len runs the launch without a prompt. */
int gitcap_dbg_argmax_final_forced(const float* amax_val, const int32_t* amax_idx, int ntiles, int rows, int row_stride, int row_off,
                                   int64_t* out, int ld_out, int32_t* sep_cnt, int step, int sep_id, const gitcap_dbg_next_embed* emb,
                                   const float* amax_sum, float* lp_out, int ld_lp, const int64_t* prompt_ids, int ld_prompt,
                                   const int32_t* lengths, int max_len, void* stream);
/* draft_accept (the accept step of gitcap_student_greedy_draft): partials [B * n][ntiles] (row r * n + j = position j of caption
 * r, n <= 63), ids int64 [B][ld] with the draft staged in columns 1..n (-1 = no word), ld >= n + 1.  a = the leading positions
 * at which every row's token equals its draft token; covered = min(a + 1, n); ids columns 1..covered and sep_cnt[0..covered - 1]
 * are rewritten from the model's tokens, nothing behind them is touched.  tok: int32 [B * n] scratch; ticket: one zero word,
 * zero again when the launch has finished.  The call synchronises `stream` and writes host_out[0] = a, host_out[1] = 1 when all
 * rows emitted sep_id in one of the covered steps, else 0 (host_out: HOST int32[2]). */
int gitcap_dbg_draft_accept(const float* amax_val, const int32_t* amax_idx, int ntiles, int B, int n, int64_t* ids, int ld,
                            int32_t* tok, uint32_t* ticket, int32_t* sep_cnt, int sep_id, int32_t* host_out, void* stream);
/* draft_accept_lp: the same launch, and lp_out[r * ld_lp + j] (fp32 [B][ld_lp], ld_lp >= n) = argmax_final_lp's value of partial row
 * r * n + j for the covered positions j < covered; nothing behind them is touched.  ids, sep_cnt and host_out as without _lp. */
int gitcap_dbg_draft_accept_lp(const float* amax_val, const int32_t* amax_idx, int ntiles, int B, int n, int64_t* ids, int ld,
                               int32_t* tok, uint32_t* ticket, int32_t* sep_cnt, int sep_id, int32_t* host_out,
                               const float* amax_sum, float* lp_out, int ld_lp, void* stream);
/* draft_accept_rows (the accept step of gitcap_greedy_draft): partials and ids as draft_accept, but every caption r keeps its own
 * a_r = leading positions whose token equals ids[r][j + 1]; covered_r = min(a_r + 1, n).  ids[r][1..covered_r] = the model's
 * tokens; len[r] (device int32 [B]) = 1 + covered_r; sep_cnt[j] += 1 (atomic; not zeroed here) for every covered (r, j) whose token
 * is sep_id; nothing behind a caption's covered part is touched.  tok int32 [B * n], row_res int32 [2 * B] scratch; ticket: 1 + B
 * zero words, zero again when the launch has finished.  The call synchronises `stream` and writes host_out (HOST int32 [4 + B]) =
 * min covered, max covered, sum of a_r, 1 when some j < min covered has sep_cnt[j] == B else 0, then a_r per caption.
 * _lp: and lp_out[r * ld_lp + j] (fp32 [B][ld_lp], ld_lp >= n) = argmax_final_lp's value of partial row r * n + j for j < covered_r. */
int gitcap_dbg_draft_accept_rows(const float* amax_val, const int32_t* amax_idx, int ntiles, int B, int n, int64_t* ids, int ld,
                                 int32_t* len, int32_t* tok, int32_t* row_res, uint32_t* ticket, int32_t* sep_cnt, int sep_id,
                                 int32_t* host_out, void* stream);
int gitcap_dbg_draft_accept_rows_lp(const float* amax_val, const int32_t* amax_idx, int ntiles, int B, int n, int64_t* ids, int ld,
                                    int32_t* len, int32_t* tok, int32_t* row_res, uint32_t* ticket, int32_t* sep_cnt, int sep_id,
                                    int32_t* host_out, const float* amax_sum, float* lp_out, int ld_lp, void* stream);
/* argmax_final_keep: the launch of a verified draft's tail step that writes position p = step + 1: a row with p < len[r] (device
 * int32 [rows], draft_accept_rows') keeps out[r] and lp_out[r] as they are, adds nothing to sep_cnt, and its emb row is embedded
 * from the id already in out[r]; every other row is gitcap_dbg_argmax_final(_lp)'s, bit for bit.  amax_sum / lp_out: both or neither. */
int gitcap_dbg_argmax_final_keep(const float* amax_val, const int32_t* amax_idx, int ntiles, int rows, int row_stride, int row_off,
                                 int64_t* out, int ld_out, int32_t* sep_cnt, int step, int sep_id, const gitcap_dbg_next_embed* emb,
                                 const float* amax_sum, float* lp_out, int ld_lp, const int32_t* len, void* stream);
/* The bookkeeping launches of the device-resident beam search over its nine state buffers (R = B * beams rows):
 * ids0 / ids1 int64 [R][max_len] (double buffered prefixes), words int64 [R], hyp_ids int64 [B][max_len], beam_scores fp32 [R],
 * hyp_score fp32 [B], src_rows int32 [R], done / hyp_len int32 [B].
 *   beam_init:   ids0[r][0] = words[r] = cls, beam_scores = 0 for the first beam of a clip and -1e9 for the others (model.py:508-509),
 *                src_rows[r] = r, done = hyp_len = 0.
 *   beam_step:   one step of model.py:573-621 on the K <= 16 sorted candidates per clip that gitcap_beam_topk wrote (every
 *                cand_idx must lie in [0, beams * V): the empty-slot sentinel of gitcap_beam_topk must not be passed on);
 *                reads ids[cur], writes ids[cur ^ 1], words, src_rows, beam_scores and the best finished hypothesis.
 *                1 <= cur_len < max_len.
 *   beam_finish: decoded int64 [B][max_len] = the best hypothesis padded with eos, logprobs fp32 [B] = its score (-1e5: none). */
typedef struct gitcap_dbg_beam_buffers {
    int64_t *ids0, *ids1, *words, *hyp_ids;
    float *beam_scores, *hyp_score;
    int32_t *src_rows, *done, *hyp_len;
} gitcap_dbg_beam_buffers;
int gitcap_dbg_beam_init(const gitcap_dbg_beam_buffers* bb, int B, int beams, int max_len, int cls, void* stream);
int gitcap_dbg_beam_step(const gitcap_dbg_beam_buffers* bb, const float* cand_scores, const int32_t* cand_idx, int B, int beams,
                         int K, int V, int cur_len, int max_len, int eos, float length_penalty, int cur, void* stream);
int gitcap_dbg_beam_finish(const gitcap_dbg_beam_buffers* bb, int B, int max_len, int eos, int64_t* decoded, float* logprobs,
                           void* stream);

/* The same bookkeeping with n hypotheses per clip (gitcap_search_options: num_keep_best; 1 <= n <= 16): hyp_ids int64
 * [B][n][max_len], hyp_score fp32 [B][n], hyp_len int32 [B][n]; the stored hypotheses of a clip sit in storage order in slots
 * 0 .. count - 1, hyp_len = 0 marks an empty slot (gitcap_dbg_beam_init on the first nine fields zeroes hyp_len[0 .. B) only: zero
 * all B * n before step 1).  beam_finish_nbest: decoded int64 [B][n][max_len], logprobs fp32 [B][n], by descending score.  With
 * n = 1 the two hooks write what gitcap_dbg_beam_step / _finish write, bit for bit. */
typedef struct gitcap_dbg_beam_buffers_nbest {
    int64_t *ids0, *ids1, *words, *hyp_ids;
    float *beam_scores, *hyp_score;
    int32_t *src_rows, *done, *hyp_len;
    int32_t n;
} gitcap_dbg_beam_buffers_nbest;
int gitcap_dbg_beam_step_nbest(const gitcap_dbg_beam_buffers_nbest* bb, const float* cand_scores, const int32_t* cand_idx, int B,
                               int beams, int K, int V, int cur_len, int max_len, int eos, float length_penalty, int cur, void* stream);
int gitcap_dbg_beam_finish_nbest(const gitcap_dbg_beam_buffers_nbest* bb, int B, int max_len, int eos, int64_t* decoded,
                                 float* logprobs, void* stream);
/* gitcap_dbg_beam_step_nbest for UNSORTED candidates (gitcap_attach_sampling: candidates), any n in [1, 16]. */
int gitcap_dbg_beam_step_sampled(const gitcap_dbg_beam_buffers_nbest* bb, const float* cand_scores, const int32_t* cand_idx, int B,
                                 int beams, int K, int V, int cur_len, int max_len, int eos, float length_penalty, int cur, void* stream);
/* The bookkeeping step of a prompted search (gitcap_attach_prompt): prompt_ids int64 [B][ld_prompt], lengths int32 [B] (clamped to
 * [1, prompt_max_len]; prompt_max_len <= ld_prompt, < max_len).  A clip with cur_len < lengths[b] is forced: ids[cur ^ 1] of each of
 * its beams = its own prefix + prompt_ids[b][cur_len], words = that token, src_rows = the identity; beam_scores, done, hyp_* and the
 * candidates of the clip are neither written nor read.  Every other clip is the plain step's, bit for bit: sampled = 0 and n = 1
 * gitcap_dbg_beam_step's kernel, n > 1 gitcap_dbg_beam_step_nbest's, sampled != 0 gitcap_dbg_beam_step_sampled's. */
int gitcap_dbg_beam_step_forced(const gitcap_dbg_beam_buffers_nbest* bb, const float* cand_scores, const int32_t* cand_idx, int B,
                                int beams, int K, int V, int cur_len, int max_len, int eos, float length_penalty, int cur, int sampled,
                                const int64_t* prompt_ids, int ld_prompt, const int32_t* lengths, int prompt_max_len, void* stream);

/* The text-row kernels of the token loop, one launcher per hook on caller-owned device buffers (tests/test_text_rows_gpu.py; a
 * plain fp64 statement of each: tests/text_rows_reference.py).  No allocation, no handle; GITCAP_ERR_ARG for arguments a launcher
 * rejects.  Weights are [Npad16][K] (rows padded to a multiple of 16), bf16, or e4m3 codes with one power-of-two scale per row.
 *   pack_frags:    dst = the fragment-major copy [tile = n / 16][k32 = k / 32][lane][8] of src [rows16][K], lane = n % 16 +
 *                  16 * ((k % 32) / 8); elem_bytes 2 (bf16) or 1 (e4m3 codes); rows16 % 16 == 0, K % 32 == 0.
 *   kv_quant_v:    the V slice of kv bf16 [rows][3 D] (columns 2 D ..) -> e4m3 codes v8 [H][pitch][64] and scales vs fp32 [H][pitch],
 *                  head-major, pitch >= rows; per (row, head) the scale is the smallest 2^e, e >= -126, with amax <= 448 * 2^e (1 for
 *                  an all-zero group), codes round to nearest even.  Rows >= `rows` of a head are not written.
 *   skinny:        out[orow(m)][n] = epi(X[m] . W[n] * wscale[n] + bias[n]) as bf16, orow(m) = (m / T) * row_stride + row_off + m % T,
 *                  n < N; epi 0 bias, 1 + erf-GELU, 2 + ReLU; K in 64, 128, 256, 576, 768, 1024 (e4m3: 128, 768).  Wpk (nullable):
 *                  the pack_frags copy of W, read instead of it.  ln_kind != 0 (M <= 2; K 64, 128, 576, 768; bf16; epi 0 or 2): X
 *                  is not read, the rows are 1: LayerNorm(sum_s ln_slabs[s][m] + ln_bias + ln_resid[m]) (slabs fp32 [nslab][M][K])
 *                  or 2: LayerNorm(ln_word[id] + ln_pos[ln_t0 + j]), id = ln_ids[(m / ln_T) * ln_ld_ids + m % ln_T] clamped into
 *                  [0, ln_vocab), j = m % ln_T; their bf16 rounding is the GEMM operand and ln_xf [M][K] receives the fp32 rows.
 *   skinny_splitk: slabs[s][m][0..N) = X[m][s Ks .. (s + 1) Ks) . W[n][the same]^T * wscale[n] (fp32 [ksplit][M][ldo], rows < M only),
 *                  Ks = K / ksplit in 32 x {1, 2, 6, 8, 12} (e4m3: 1, 2, 12); ksplit 0 = the launcher's default; N % 16 == 0.
 *   ln_reduce:     xf / xb [M][D] = LayerNorm(sum_s slabs[s][m] + bias + resid[m]) as fp32 / bf16; nslab 1..64, D % 4 == 0, <= 1024.
 *   ffn_txt:       slabs[s][m][0..D) = h[m][64 s .. 64 s + 63] . W2[:, the same]^T, h = bf16(erf-GELU(X W1^T + b1)); W1pk / W2pk the
 *                  pack_frags copies of W1 [F][D] / W2 [D][F] (bf16, or e4m3 with w1scale [F] / w2scale [D]); D 128 or 768, F % 64 == 0.
 *   txt_block:     the attention sub-layer of M = rows * T text rows (a plain-C mirror of TxtBlockArgs; csrc/kernels.h).  Query m =
 *                  (r, j) at position t0 + j reads q from kv_txt [rows][Tmax][3 D] (q | k | v) and attends the S_img image keys of clip
 *                  r / beams in kv_img [clips * S_img][3 D] and the text keys 0 .. t0 + j of row r, scale 1/8, H = D / 64 heads; with
 *                  v8_img / vs_img (kv_quant_v's output, pitch v8_pitch >= clips * S_img) the image V is code * scale.  part [M][H][D]
 *                  = bf16(ctx_h) . aow[:, 64 h .. 64 h + 63]^T per head (aow [D][D] bf16, aowpk its pack_frags copy or NULL; or e4m3
 *                  codes with aoscale [D], aowpk ignored); xs / xsb [M][D] = LayerNorm(sum_h part + aob + xin) as fp32 / bf16.  cnt [M]
 *                  are the arrival tickets: zero before the first launch, zero again after every launch.  nt_kv: non-temporal K/V
 *                  loads (same bits).  D 128 or 768; t0 + T <= Tmax. */
int gitcap_dbg_pack_frags(const void* src, void* dst, int rows16, int K, int elem_bytes, void* stream);
int gitcap_dbg_kv_quant_v(const void* kv, void* v8, float* vs, int rows, int D, int H, int64_t pitch, void* stream);
typedef struct gitcap_dbg_skinny_args {
    const void* X;
    int32_t ldx;
    const void *W, *Wpk;
    const float *wscale, *bias;
    int32_t M, N, K;
    void* out;
    int32_t ldo, T, row_stride, row_off;
    int32_t ln_kind;
    const float* ln_slabs;
    int32_t ln_nslab;
    const float *ln_bias, *ln_resid;
    const int64_t* ln_ids;
    int32_t ln_ld_ids, ln_T, ln_t0, ln_vocab;
    const float *ln_word, *ln_pos, *ln_g, *ln_b;
    float ln_eps;
    float* ln_xf;
} gitcap_dbg_skinny_args;
int gitcap_dbg_skinny(const gitcap_dbg_skinny_args* a, int epi, void* stream);
int gitcap_dbg_skinny_splitk(const void* X, int ldx, const void* W, const void* Wpk, const float* wscale, int M, int N, int K, int ksplit,
                             float* slabs, int ldo, void* stream);
int gitcap_dbg_ln_reduce(const float* slabs, int nslab, const float* bias, const float* resid, const float* gamma, const float* beta,
                         float eps, int M, int D, float* xf, void* xb, void* stream);
int gitcap_dbg_ffn_txt(const void* X, int ldx, const void* W1pk, const void* W2pk, const float* w1scale, const float* w2scale,
                       const float* b1, int M, int D, int F, float* slabs, void* stream);
typedef struct gitcap_dbg_txt_block_args {
    const void *kv_img, *kv_txt;
    int32_t rows, beams, t0, T, Tmax, S_img, H, D;
    const void *aow, *aowpk;
    const float *aoscale, *aob, *g1, *b1, *xin;
    float eps;
    float* part;
    uint32_t* cnt;
    float* xs;
    void* xsb;
    const void* v8_img;
    const float* vs_img;
    int64_t v8_pitch;
    int32_t nt_kv;
} gitcap_dbg_txt_block_args;
int gitcap_dbg_txt_block(const gitcap_dbg_txt_block_args* a, void* stream);
/* txt_block, variable-length form: clip c = row / beams has its image keys at rows off[c] .. off[c] + len[c] - 1 of the packed
 * kv_img (and of v8_img / vs_img); off, len device int32 [ceil(rows / beams)]; S_img is not read.  A row's outputs are bit for bit
 * gitcap_dbg_txt_block's with S_img = len[c] on that clip's keys. */
int gitcap_dbg_txt_block_varlen(const gitcap_dbg_txt_block_args* a, const int32_t* off, const int32_t* len, void* stream);

/* The staging and layout kernels between those: csrc/preproc.hip, the plain row kernels of csrc/rowops.hip and the text embedding
 * of csrc/select.hip, one launcher per hook on caller-owned device buffers (tests/test_staging_gpu.py; a plain fp64 statement of each: tests/staging_reference.py).
 * No handle, no allocation; GITCAP_ERR_ARG, before any launch, for null pointers, misaligned pointers and sizes that would index
 * outside a buffer.  (gitcap_preprocess is the fp32 form of the transform and needs no hook.)
 *   preprocess_patches: gitcap_preprocess's transform fused with the patch gather -> bf16 rows [nf * (crop / p)^2][Kp], column
 *                  c * p * p + py * p + px; columns >= 3 p^2 are NOT written.  crop % p == 0, Kp >= 3 p^2, Kp % 2 == 0.
 *   preprocess_stem: the transform fused with the gather of a 3x3 stride-2 pad-1 convolution -> bf16 rows [nf * (crop / 2)^2][32],
 *                  column ci * 9 + ky * 3 + kx, every column written (zero at taps outside the frame and at columns >= 27).  crop even,
 *                  col 16-byte aligned.
 *   im2col:        frames fp32 [nf][3][img][img] -> bf16 rows [nf * (img / p)^2][Kp], the same columns, zero from 3 p^2 on.  img % p == 0,
 *                  p even, Kp >= 3 p^2; p % 4 == 0 and img % 4 == 0: Kp % 4 == 0, frames 16-byte and patches 8-byte aligned; else
 *                  Kp % 2 == 0 and 4-byte alignment.
 *   cast_bf16:     out bf16 [n] = in fp32 [n], round to nearest even; n % 4 == 0.
 *   dequant_fp8:   out bf16 [rows][K] = e4m3 code w8[r][k] * scale[r] (a power of two: exact); K % 16 == 0.
 *   dequant_fp8_batch: n <= 4 such matrices in one launch; the five arguments are HOST arrays of n entries.
 *   embed_text:    row m = (r, j), r < rows, j < T: xf fp32 / xb bf16 [rows * T][D] = LayerNorm(word[id] + pos[t0 + j]) * gamma + beta,
 *                  id = ids[r * ld_ids + j] clamped into [0, vocab).  Either of xf / xb may be NULL.  D % 4 == 0, D <= 1024, ld_ids >= T.
 *   window_scatter: src fp32 [B][n][rows_per_frame][D] -> ring [B][F][rows_per_frame][D], frame j of clip b to slot (head + j) % F;
 *                  no other slot is written.  n <= F, head < F, D % 4 == 0.
 *   window_assemble: row (b, f, tok) of out bf16 [B * F * N][D] = ring[b][(head + f) % F][tok] + temporal[f] (fp32 add, then rounded);
 *                  vis (nullable) = the fp32 sum; temporal (nullable) fp32 [F][D].  D % 4 == 0, D <= 1024.
 *   ragged_tables: counts = HOST int32 [B], 1 .. 255 each, B <= 256: off[b] = N * sum_{i < b} counts[i], len[b] = N * counts[b],
 *                  pos[frame] = the frame's index inside its clip; pos_cap = the entries pos holds (>= the sum of the counts).
 *   ragged_temporal: row r of out bf16 [frames * N][D] = ln[r] + temporal[pos[r / N]], vis (nullable) the fp32 sum; pos is read back
 *                  first: an entry outside [0, temporal_rows) is refused.
 *   pool_plan:     touches no device.  The stream pool's host plan (csrc/host_logic.h: pool_plan) on n_streams cursors of F slots,
 *                  heads / counts HOST int32 [n_streams] (in and out: the push advances them).  First the push: frame i of push_ids
 *                  [n_push] -> ring frame dst[i] = stream * F + slot.  Then the call on the cursors behind it: row r = stream
 *                  cap_ids[r] [B]; src / pos [sum of the rows' counts] = each packed frame's ring frame and index inside its own
 *                  clip, off / len [B] = each row's first packed frame and frame count; out3 = {packed frames, longest row, dense}.
 *                  n_push = 0 / B = 0 leave a half out (its pointers may be NULL).  GITCAP_ERR_ARG: a stream id out of range, more
 *                  than F frames for one stream, a stream named twice; GITCAP_ERR_STATE: a named stream holds nothing.  A refused
 *                  plan writes nothing.
 *   pool_scatter:  frame i of stage fp32 [frames][N][D] -> ring frame dst[i] of ring [ring_frames][N][D]; no other row is written.
 *                  dst (device int32 [frames]) is read back first: an entry outside [0, ring_frames) or one that repeats is refused.
 *   pool_assemble: row (g, tok) of out bf16 [frames * N][D] = ring[src[g]][tok] + temporal[pos[g]] (temporal nullable: no add, pos
 *                  unused); src / pos (device int32 [frames]) are read back first and checked against ring_frames / temporal_rows. */
int gitcap_dbg_pool_plan(int n_streams, int F, int32_t* heads, int32_t* counts, const int32_t* push_ids, int n_push, int32_t* dst,
                         const int32_t* cap_ids, int B, int32_t* src, int32_t* pos, int32_t* off, int32_t* len, int32_t* out3);
int gitcap_dbg_pool_scatter(const float* stage, float* ring, int ring_frames, const int32_t* dst, int frames, int N, int D, void* stream);
int gitcap_dbg_pool_assemble(const float* ring, int ring_frames, const float* temporal, int temporal_rows, const int32_t* src,
                             const int32_t* pos, void* out, int frames, int N, int D, void* stream);
/*   gather_hidden: out[b][e][s][:] = s < S_img ? img[e][b * S_img + s][:] : txt[e][b * T + s - S_img][:], e < n_entries, fp32 rows of D;
 *                  entry e of img / txt starts e * the entry stride (in floats, % 4 == 0) behind the first.  D % 4 == 0.
 *   gather_txt_rows: dst[l][r][t][:] = src[l][src_rows[r]][t][:], t < t_len, l < layers, bf16 rows of `width`, rows [.][Tmax][width],
 *                  layers layer_stride elements apart; copied in pieces of 8 elements: t_len * width, Tmax * width and layer_stride
 *                  are multiples of 8; t_len <= Tmax; src_rows (device int32 [rows], read back first) in [0, rows). */
int gitcap_dbg_preprocess_patches(const uint8_t* frames_hwc_bgr, int nf, int H, int W, int crop, int p, int Kp, void* patches, void* stream);
int gitcap_dbg_preprocess_stem(const uint8_t* frames_hwc_bgr, int nf, int H, int W, int crop, void* col, void* stream);
int gitcap_dbg_im2col(const float* frames, int nf, int img, int p, int Kp, void* patches, void* stream);
int gitcap_dbg_cast_bf16(const float* in, void* out, int64_t n, void* stream);
int gitcap_dbg_dequant_fp8(const void* w8, const float* scale, void* out, int rows, int K, void* stream);
int gitcap_dbg_dequant_fp8_batch(int n, const void* const* w8, const float* const* scale, void* const* out, const int32_t* rows,
                                 const int32_t* K, void* stream);
int gitcap_dbg_embed_text(const int64_t* ids, int ld_ids, int rows, int T, int t0, const float* word, const float* pos, const float* gamma,
                          const float* beta, float eps, int D, int vocab, float* xf, void* xb, void* stream);
int gitcap_dbg_window_scatter(const float* src, float* ring, int B, int n, int F, int head, int rows_per_frame, int D, void* stream);
int gitcap_dbg_window_assemble(const float* ring, const float* temporal, void* out, float* vis, int B, int F, int head, int N, int D,
                               void* stream);
int gitcap_dbg_ragged_tables(const int32_t* counts, int B, int N, int32_t* off, int32_t* len, int32_t* pos, int pos_cap, void* stream);
int gitcap_dbg_ragged_temporal(const float* ln, const float* temporal, int temporal_rows, const int32_t* pos, void* out, float* vis,
                               int frames, int N, int D, void* stream);
int gitcap_dbg_gather_hidden(const float* img, const float* txt, float* out, int n_entries, int B, int S_img, int T, int D,
                             int64_t img_entry_stride, int64_t txt_entry_stride, void* stream);
int gitcap_dbg_gather_txt_rows(const void* src, void* dst, const int32_t* src_rows, int rows, int t_len, int Tmax, int width, int layers,
                               int64_t layer_stride, void* stream);

/* The TinyViT encoder's kernels (csrc/tinyvit.hip) and the student decoder's attention (csrc/student.hip), one kernel per hook on
 * caller-owned device buffers (tests/test_encoder_kernels_gpu.py; a plain fp64 statement of each: tests/encoder_kernels_reference.py).
 * No handle, no weight upload; GITCAP_ERR_ARG for arguments the launcher refuses, before any launch.  Activations are bf16.
 *   tv_gemm:    out[m][n] = epi(A[m] . W[n] + bias[n]), A [M][lda], W [N][K], bias fp32 [N], res [M][ldr], out [M][ldo]; epi 0, 1 (erf-GELU),
 *               2 (+ res), 2 | 4 (+ res, then erf-GELU); res may be out.  N % 4 == 0, K % 32 == 0, lda % 8 == 0, ldo % 4 == 0, ldr % 4 == 0.
 *   tv_im2col:  the 3x3 stride-2 pad-1 patches of the stem convolutions: out [n * H/2 * W/2][Kp], column ci * 9 + ky * 3 + kx, zero for
 *               columns >= 9 Cin; in: fp32 NCHW [n][Cin][H][W] (f32_nchw != 0) or bf16 NHWC [n][H][W][Cin].  H, W even, Kp >= 9 Cin.
 *   tv_dwconv:  depthwise 3x3, pad 1, stride 1 or 2, + bias (+ erf-GELU): x [n][H][W][C] -> out [n][H/stride][W/stride][C]; w9 is the
 *               device layout fp32 [9][C] (tap ky * 3 + kx major).  C % 8 == 0; stride 2 needs even H and W.
 *   tv_ln:      LayerNorm of the rows of x [M][C] -> out [M][C]; g, b fp32 [C].  C % 8 == 0, C <= 2048.
 *   tv_attn:    windowed attention of qkv [n * H * W][3 * 32 * heads] (head h's q | k | v at columns 96 h + {0, 32, 64}) -> ctx
 *               [n * H * W][32 * heads], windows of ws x ws pixels, scale 32^-1/2.  attention_biases: the COMPACT checkpoint table, device
 *               fp32 [heads][ws * ws]; the hook expands it to the dense [heads][ws^2][ws^2] table with the function
 *               gitcap_tinyvit_finalize uses, launches, synchronises `stream` and frees the table.  1 <= ws <= 14, H % ws == W % ws == 0.
 *   tv_pool:    mem fp32 [n][C] = the mean over the HW rows of x [n][HW][C].
 *   tv_to_nchw: out fp32 [n][C][HW] = x [n][HW][C].
 *   attn_small: a plain-C mirror of SmallAttnArgs (csrc/kernels.h), passed to launch_attn_small: query m = (r, j), r = m / T, reads q at
 *               row r * q_row_stride + q_row_off + j (ldq columns per row), head h at columns h * hd; key / value i of row r at row
 *               r * keys_stride + i of k / v (ldkv); nkeys > 0: keys 0 .. nkeys - 1, nkeys == 0: causal, keys 0 .. t0 + j; ids (nullable):
 *               key i of row r is masked when ids[r * ld_ids + i] == pad_id (every key masked: NaN); ctx [M][ldc].  At most 64 keys,
 *               hd % 8 == 0, hd <= 128, ldkv % 8 == 0. */
int gitcap_dbg_tv_gemm(const void* A, int lda, const void* W, const float* bias, const void* res, int ldr, void* out, int ldo, int M,
                       int N, int K, int epi, void* stream);
int gitcap_dbg_tv_im2col(const void* in, int f32_nchw, void* out, int n, int H, int W, int Cin, int Kp, void* stream);
int gitcap_dbg_tv_dwconv(const void* x, const float* w9, const float* bias, void* out, int n, int H, int W, int C, int stride, int gelu,
                         void* stream);
int gitcap_dbg_tv_ln(const void* x, const float* g, const float* b, void* out, int M, int C, float eps, void* stream);
int gitcap_dbg_tv_attn(const void* qkv, const float* attention_biases, void* ctx, int n, int H, int W, int heads, int ws, void* stream);
int gitcap_dbg_tv_pool(const void* x, float* mem, int n, int HW, int C, void* stream);
int gitcap_dbg_tv_to_nchw(const void* x, float* out, int n, int HW, int C, void* stream);
typedef struct gitcap_dbg_attn_small_args {
    const void* q;
    int32_t ldq, T, q_row_stride, q_row_off;
    const void *k, *v;
    int32_t ldkv, keys_stride, nkeys, t0;
    const int64_t* ids;
    int32_t ld_ids, pad_id;
    void* ctx;
    int32_t ldc;
    int32_t M, H, hd;
} gitcap_dbg_attn_small_args;
int gitcap_dbg_attn_small(const gitcap_dbg_attn_small_args* a, void* stream);
/* The variable-length form the student's cross-attention takes for clips of different length (gitcap_student_attach_frame_counts):
 * k | v are PACKED and the keys of text row r are rows key_off[r] .. key_off[r] + key_len[r] - 1 of them (device int32 [M / T] each,
 * 1 <= key_len <= 64).  nkeys, keys_stride and t0 of the struct are not read; ids must be NULL.  A row with key_len = n holds the bits
 * of gitcap_dbg_attn_small at nkeys = n on that row's keys.  Synchronises `stream` (the tables are checked on the host first). */
int gitcap_dbg_attn_small_varlen(const gitcap_dbg_attn_small_args* a, const int32_t* key_off, const int32_t* key_len, void* stream);

/* Residual stream of the ViT per block (tests/test_stress_layers_gpu.py: single-block checks on the device's own inputs).
 * While `buf` is non-NULL every SYNCHRONOUS image pass (gitcap_encode / _greedy / _beam_search and their _raw forms) copies
 * the fp32 residual stream x [rows][enc_width] (rows = B * F * tokens per frame, unpadded) to buf + e * rows * enc_width:
 * e = 0 the ln_pre output, e = i the output of encoder block i - 1, for e < enc_layers (the last block's output only exists
 * behind ln_post: visual_out of gitcap_encode).  buf: device fp32 [enc_layers][rows][enc_width], caller owned; NULL disables. */
int gitcap_dbg_enc_tap(gitcap_t* h, float* buf);

/* Introspection used by tests and bench.py.  gitcap_weight_bytes counts the tensors as loaded; the fragment-major second copies of
 * the decoder / head weights that gitcap_finalize_weights makes for the token loop (+132 MB bf16 / +66 MB e4m3 at GIT-base), the
 * e4m3 staging panels and everything sized by max_batch / max_frames / max_text_len / max_beams are workspace.  The text-row
 * scratch of the four pipeline slots grows with rows = max_batch * max_beams * max_text_len: 48 fp32 FC2 slabs + 12 per-head
 * partials per row = 184 KB per row and slot (INTEGRATION.md par. 4 has the formula). */
int gitcap_workspace_bytes(const gitcap_t* h, int64_t* bytes);
int gitcap_abi_version(void);

/* ---------------------------------------------------------------------------------------------------
 * Student decoder (SURVEY.md par. 8 row f.2): StudentCandidateV1, src/models/model.py:50-187 --
 * torch.nn.TransformerDecoder (post-LN, ReLU; model.py:82-85) over the caption so far (causal mask,
 * PAD tokens masked as keys; model.py:134-136, src/utils/masking.py) with cross-attention over
 * `memory` = one token per frame (model.py:124), embedding + positional table / sqrt(d_model)
 * (model.py:140-144, :320-340) and a Linear vocabulary head (model.py:152).  The TinyViT image encoder
 * (timm, model.py:38) has its own handle below (gitcap_tinyvit_*); the decoder takes memory [B][mem_tokens][d_model].
 * Tensor names are the reference's state_dict keys (embed.weight, pos_enc.pe,
 * decoder.layers.{i}.self_attn.in_proj_weight, ..., linear.weight, linear.bias); same ownership, error
 * and threading rules as the gitcap_* entry points above.
 * ------------------------------------------------------------------------------------------------- */
typedef struct gitcap_student gitcap_student_t;
struct gitcap_student_config {
    int32_t d_model, n_head, d_ffn, num_layers;      /* config.py:79-83: 576, 8, 1024, 2 */
    int32_t vocab_size, cls_token_id, sep_token_id;  /* 30522, 101, 102 */
    int32_t pad_token_id;                            /* 0: create_padding_mask default, masking.py:4 */
    int32_t mem_tokens;                              /* frames per clip (6) */
    int32_t max_pos;                                 /* rows of the positional table (500, model.py:324) */
    int32_t max_rows;                                /* largest batch the workspace is sized for */
    int32_t max_text_len;                            /* largest max_len of greedy / T-1 of forward_decoder (<= 63) */
    float ln_eps;                                    /* 1e-5 */
};
/* StudentCandidateV1.__init__ (model.py:55-106) for the decoder part */
int gitcap_student_create(const struct gitcap_student_config* cfg, int device, gitcap_student_t** out);
void gitcap_student_destroy(gitcap_student_t* h);
const char* gitcap_student_last_error(const gitcap_student_t* h);
/* load_state_dict (src/inference.py:38): host fp32 data, logical shape; GEMM weights are stored as bf16 */
int gitcap_student_load_tensor(gitcap_student_t* h, const char* name, const float* data, const int64_t* shape, int rank);
int gitcap_student_finalize(gitcap_student_t* h);
/* memory: device fp32 [B][mem_tokens][d_model] (model.py:124) -> bf16 + the cross-attention K/V of every layer */
int gitcap_student_set_memory(gitcap_student_t* h, const float* memory, int B, void* stream);
/* forward_decoder (model.py:128-154): ids device int64 [B][ld_ids] (T valid columns) -> logits device fp32
 * [B][T][vocab].  Needs a preceding set_memory with the same B.  A row whose first token is PAD yields NaN
 * for that position, as torch does (every key masked). */
int gitcap_student_forward_decoder(gitcap_student_t* h, const int64_t* ids, int ld_ids, int B, int T, float* logits, void* stream);
/* greedy_decode (model.py:156-187) from memory: ids_out device int64 [B][max_len+1], CLS-prefixed; the
 * token loop runs on the device with an exact KV cache; steps_out (device int32[1], nullable) = number of
 * generated tokens under the stop rule (enum gitcap_stop; GITCAP_STOP_ALL_SEP = model.py:184). */
int gitcap_student_greedy(gitcap_student_t* h, const float* memory, int B, int max_len, int stop,
                          int64_t* ids_out, int32_t* steps_out, void* stream);
/* StudentCandidateV1.beam_search (src/models/model.py:189-318) on the device, KV-cached, no host round trip: memory [B][F][D] fp32
 * (device), k beams (rows b * k + i; B * k <= max_rows, k <= 16), no end-of-sequence handling (as the reference);
 * ids_out [B][max_len] = the best beam of every clip, CLS first (model.py:317). */
int gitcap_student_beam_search(gitcap_student_t* h, const float* memory, int B, int k, int max_len, int64_t* ids_out, void* stream);

/* Memory-token window: the live loop of the reference (src/real_time_inference.py:30-57 collects six transformed frames, calls
 * greedy_decode on all six, clears the list) as a sliding window that computes everything belonging to a frame once.  A memory
 * token is one frame's own stage-3 mean (model.py:124) and its cross-attention K | V rows in every decoder layer are
 * W_kv . token + b with no positional term, so a push computes them for the n new tokens only -- set_memory's GEMM on B * n rows
 * instead of B * mem_tokens -- and keeps them in a ring of mem_tokens slots per clip; a window call copies the ring's rows, oldest
 * first, to where set_memory would have written them and runs the token loop of the full call (the same captured graph).
 * Contract: gitcap_student_window_greedy / _beam_search return bit for bit what gitcap_student_greedy / _beam_search return on the
 * window's mem_tokens tokens in push order (a K | V row has the same bits whichever launch computed it: one MFMA chain per row).
 *   reset  B clips (<= max_rows) advance in lockstep; allocates the ring (bf16 [num_layers][B][mem_tokens][2 d_model]) and a
 *          staging buffer of B * mem_tokens rows, empties the window; B = 0 releases both (so does destroy).  A handle that never
 *          resets a window allocates nothing.  Changing B waits for the device before the old ring is freed.
 *   push   memory: device fp32 [B][n][d_model], 1 <= n <= mem_tokens, token j older than token j + 1 -- the `memory` output of
 *          gitcap_tinyvit_encode(_raw).  Writes the ring and the staging buffer only: not the memory K | V of the decoder, not the
 *          self-attention cache, not the current row count, so a gitcap_student_forward_decoder after a push still sees the
 *          previous memory.
 *   window calls  need mem_tokens tokens pushed since the reset; leave the handle as the full call would (a forward_decoder
 *          after one sees the window; for beam search with B * k rows).  Arguments as the full calls without memory / B.
 * Pushes and window calls may be issued on different streams: two events order a push behind the last window call's copy and
 * the last push, and a window call behind the last push; there is no device synchronisation on the data path.
 * Errors: GITCAP_ERR_ARG for a null handle or pointer, B different from the reset's, n outside [1, mem_tokens], B > max_rows at
 * reset, B * k > max_rows, and the length / stop-rule checks of the full calls; GITCAP_ERR_STATE for a push before any reset, a
 * window call before mem_tokens tokens have been pushed since the reset, and weights not finalized. */
int gitcap_student_window_reset(gitcap_student_t* h, int B);
int gitcap_student_window_push(gitcap_student_t* h, const float* memory, int B, int n, void* stream);
int gitcap_student_window_greedy(gitcap_student_t* h, int max_len, int stop, int64_t* ids_out, int32_t* steps_out, void* stream);
int gitcap_student_window_beam_search(gitcap_student_t* h, int k, int max_len, int64_t* ids_out, void* stream);

/* Greedy decoding that verifies a draft caption in one pass (self-speculative greedy; the reference has no counterpart: its live
 * loop re-runs greedy_decode from [CLS] on every window, src/real_time_inference.py:56-61).  Two consecutive windows of a live stream
 * share all but `hop` frames, so the previous caption is a good guess at the next.  The cached token loop equals one teacher-forced
 * pass over its own output bit for bit and a row does not depend on the rows beside it, so one pass over the draft's n_draft
 * positions -- the launches of one token step -- yields every token the loop would emit after each draft prefix: the leading draft
 * tokens that equal them are accepted (all rows in lockstep: the minimum over the rows), the first position that differs already
 * holds the loop's own token, and only the steps behind it are decoded one by one (replayed from per-step graphs captured at the
 * first draft call of a (B, max_len, speed switches)).
 *   draft_ids  device int64 [B][ld_draft]: column 0 is ignored and taken as CLS, columns 1..n_draft are the guessed tokens,
 *              1 <= n_draft <= max_len, ld_draft >= n_draft + 1 (e.g. the ids_out of the previous call)
 *   accepted_out  host int32 (nullable): the number of leading draft tokens accepted, 0..n_draft
 *   the other arguments as gitcap_student_greedy / gitcap_student_window_greedy
 * Contract: ids_out[:, :1 + steps] and *steps_out are bit for bit those of gitcap_student_greedy / _window_greedy with the same
 * arguments, whatever the draft holds -- PAD, SEP, ids outside [0, vocab) and negative ids included: such an id is never used as an
 * index (it is staged as "no word" on the device, its embedding lookup is clamped to the table) and can only mismatch, so the row is
 * accepted up to that position at most.  Under GITCAP_STOP_NEVER steps = max_len and every column is defined; under
 * GITCAP_STOP_ALL_SEP the columns beyond 1 + steps are unspecified.  The call leaves the handle as the full call would (a
 * gitcap_student_forward_decoder after it sees the same memory) and does not touch the full loop's captured graphs.
 * These are the only student data-path calls that wait on the host: for an event recorded behind the verify pass on `stream` (the
 * accepted count decides which steps are enqueued), never for the device.
 * Errors: GITCAP_ERR_ARG for a null handle, draft_ids or ids_out, n_draft < 1, n_draft > max_len, ld_draft < n_draft + 1, and the
 * length / stop-rule / B / window-state errors of the calls they shadow (GITCAP_ERR_STATE for a window call before mem_tokens pushes).
 * gitcap_student_draft_stats: host int64[4] = draft calls, draft tokens offered (n_draft summed), tokens accepted, tail steps
 * enqueued, since the handle was created. */
int gitcap_student_greedy_draft(gitcap_student_t* h, const float* memory, int B, const int64_t* draft_ids, int ld_draft, int n_draft,
                                int max_len, int stop, int64_t* ids_out, int32_t* steps_out, int32_t* accepted_out, void* stream);
int gitcap_student_window_greedy_draft(gitcap_student_t* h, const int64_t* draft_ids, int ld_draft, int n_draft, int max_len, int stop,
                                       int64_t* ids_out, int32_t* steps_out, int32_t* accepted_out, void* stream);
int gitcap_student_draft_stats(const gitcap_student_t* h, int64_t* out4);
/* Per-token log-probabilities of the student's greedy captions: gitcap_attach_token_logprobs for this handle.  One-shot; consumed
 * by the next of gitcap_student_greedy, gitcap_student_window_greedy, gitcap_student_greedy_draft, gitcap_student_window_greedy_draft
 * (success or failure); other entry points leave it pending; NULL detaches.  logprobs_out: device fp32 [B][ld], ld >= max_len,
 * column t = the natural-log probability of ids_out[b][t + 1]; columns < *steps_out defined (the draft forms may stop on the
 * host), columns >= max_len not written.  With a draft the covered positions come from the verify pass and the rest from the tail
 * steps: by the exact-KV-cache property the values are bit for bit those of the plain call.  Needs finalized weights
 * (GITCAP_ERR_STATE); GITCAP_ERR_ARG for ld < 1 or a misaligned pointer, and at the consuming call for ld < max_len (nothing
 * launched, attachment consumed).  The first attach allocates the third partial (sized as the arg-max partials, which covers
 * the verify pass's B * n_draft rows) and the handle's own [rows][max_len] staging the captured loops write. */
int gitcap_student_attach_token_logprobs(gitcap_student_t* h, float* logprobs_out, int ld);
/* gitcap_attach_top_logprobs for this handle: same layout ([B][ld][k]), order, tie rule and -1 / -inf padding.  One-shot; taken by
 * the next of gitcap_student_greedy, gitcap_student_window_greedy and gitcap_student_score; gitcap_student_greedy_draft and
 * gitcap_student_window_greedy_draft consume it and fail with GITCAP_ERR_ARG and a message that names it; beam search leaves it
 * pending.  Needs finalized weights.  The captured token loop is keyed by k; the first attach allocates the third partial and the
 * handle's own [rows][max_len][32] staging the captured loops write. */
int gitcap_student_attach_top_logprobs(gitcap_student_t* h, int k, int64_t* top_ids, float* top_lp, int ld);
/* Constrained decoding on the student: gitcap_attach_constraints for this handle -- the same struct (suppress is a device int32
 * list), the same banned set per row and step (prefix = the row's ids so far, CLS included; the SEP of min_length is the handle's
 * sep_token_id), banned columns -inf ahead of the arg-max, the log-probabilities, the alternatives and the log-softmax of the beam
 * ranking.  The student's loops keep decoding behind a row's SEP, and the rules keep applying there.
 * A ONE-SHOT attachment with the life cycle of gitcap_attach_constraints: the next call of the greedy family (gitcap_student_greedy,
 * _window_greedy, _window_greedy_partial, _pool_greedy) or of the beam family (gitcap_student_beam_search, _window_beam_search)
 * consumes it, whichever comes first, whether that call succeeds or is refused; gitcap_student_greedy_draft and
 * _window_greedy_draft consume it and fail with GITCAP_ERR_ARG; gitcap_student_score, _attention, _forward_decoder, _set_memory, the
 * pushes and gitcap_distill leave it pending; NULL detaches.  It combines with the log-probability, top-logprob and frame-count
 * attachments.  In a pool call one set of rules applies to every stream named.
 * The greedy loops are captured graphs, so the rules are no kernel arguments: the consuming call writes them to a device record
 * (int32 [4 + 256]: n, min_length, n_suppress, 0, the ids) on the caller's stream ahead of the replay -- `suppress` is read by a
 * device-to-device copy enqueued there, at the consuming call -- and every step's mask launch reads the record when it runs.  One
 * captured loop per (B, max_len, ...) serves every set of rules; a call without constraints replays the unconstrained loop.
 * The first attach allocates the mask (uint16 [max_rows][ld], ld even >= ceil(V / 16)), the record and a page-locked copy of its
 * header; a handle that never attaches allocates nothing and runs exactly the launches it ran before.
 * Errors, all GITCAP_ERR_ARG: a negative field; n_suppress > 256; n_suppress > 0 with a null or misaligned pointer; a vocabulary
 * above 131072 columns; at the consuming call n_suppress + max_len >= vocab_size (greedy) or n_suppress + max_len + k > vocab_size
 * (beam).  Nothing is launched then and the attachment is consumed all the same.  GITCAP_ERR_STATE before the weights are finalized. */
int gitcap_student_attach_constraints(gitcap_student_t* h, const gitcap_constraints* c);
/* Prompted decoding on the student: gitcap_attach_prompt for this handle -- the same arguments (prompt_ids device int64 [B][ld] with
 * CLS at column 0, lengths device int32 [B] = valid tokens per clip, CLS included, 1 = no prompt for that clip; min_len / max_len
 * the host's minimum and maximum of lengths; NULL / NULL detaches), the same clamp (the kernels clamp lengths[b] to [1, max_len] of
 * the consuming call, so a mismatch reads nothing outside a table row) and the same treatment of ids outside the vocabulary.
 * A ONE-SHOT attachment with the life cycle of gitcap_attach_prompt: the next call of the greedy family (gitcap_student_greedy,
 * _window_greedy, _window_greedy_partial, _pool_greedy) or of the beam family (gitcap_student_beam_search, _window_beam_search)
 * consumes it, whichever comes first, whether that call succeeds or is refused; gitcap_student_greedy_draft and
 * _window_greedy_draft consume it and fail with GITCAP_ERR_ARG; every other entry point leaves it pending.  It combines with the
 * log-probability, top-logprob, frame-count and constraint attachments.  In a window call row b is clip b of the window, in a pool
 * call row r is the stream stream_ids[r] names.
 * The greedy loops are captured graphs, so the prompt is no kernel argument: the consuming call copies the caller's rows (max_len
 * columns each, and the lengths) into tables the handle owns -- int64 [max_rows][max_text_len + 2] and int32 [max_rows] --, device to
 * device on the caller's stream ahead of the replay, and the captured nodes name only those tables.  The caller's buffers are read
 * by those copies and may be reused once they have run.
 * Greedy: a small staging launch takes the place of the CLS fill: row r = CLS, the prompt's tokens 1 .. lengths[r] - 1, CLS behind
 * them -- the whole prompt stands in the id rows before the first position runs, because the self-attention masks PAD keys by id.
 * Every step then runs the forced form of the arg-max against the tables: a row whose prompt covers the position written takes
 * the prompt's token (for the output and the next step's input), the token is not counted by the stop rule, 0.0f is written for
 * its log-probability, and it is emitted even when a constraint bans it; attached top-k alternatives still report the model's own
 * ranks there.  Positions 0 .. min_len - 1 are prompt in every row: with min_len >= 2 they run as ONE pass (the head on its last
 * position only, the arg-max forced at position min_len) unless constraints or top-k alternatives are attached, which need every
 * position's step; the prompt then runs as forced token steps (same ids: a cached step is bit for bit the teacher-forced
 * position).  The captured loop is keyed by that plan -- 0 unprompted, 1 forced steps, min_len for one pass -- so one graph serves
 * every prompt of its plan, and a call without a prompt replays the loop it replayed before.  ids_out includes the prompt.
 * Beam: the rows start from the staged prompts (clip b's row for its k beams); while t + 1 < lengths[b] the bookkeeping step does
 * not rank clip b: every one of its k rows keeps its own prefix and appends prompt_ids[b][t + 1], src_rows is the identity and the
 * scores stay untouched, so a clip leaves its prompt with [0, -1e9, ..] as it leaves CLS.  max_len counts the prompt; the search
 * keeps its semantics otherwise (no end-of-sequence handling).  The beam rows take no multi-position pass.
 * Errors: GITCAP_ERR_ARG for one null pointer, a misaligned pointer, min_len < 1, max_len < min_len, ld < max_len or max_len >
 * max_text_len + 1; GITCAP_ERR_STATE before the weights are finalized; at the consuming call max_len > the call's max_len (greedy) or
 * > max_len - 1 (beam: at least one free position) gives GITCAP_ERR_ARG with nothing launched (the attachment is consumed all the
 * same).  The first attach allocates the two tables; a handle that never attaches allocates nothing and makes the launches it made. */
int gitcap_student_attach_prompt(gitcap_student_t* h, const int64_t* prompt_ids, int ld, const int32_t* lengths, int min_len, int max_len);
/* Beam search that ends hypotheses at SEP: the search of gitcap_beam_search (GeneratorWithBeamSearchV2, model.py:479-678) on the
 * student, in the place of the reference's unfinished loop (model.py:189-318, end-of-sequence handling commented out).  With this
 * attachment a call of the beam family (gitcap_student_beam_search, _window_beam_search, _pool_beam_search) ranks k *
 * per_node_beam_size candidates per clip and step; a candidate that is SEP, or any candidate of the last step, finishes the
 * hypothesis ids[0 .. cur_len) with score = sum of log-probabilities (the finishing token's included) / cur_len^length_penalty; a
 * clip keeps its num_keep_best best and is done once its worst kept score >= the best candidate sum / (max_len - 1)^length_penalty.
 * A done clip's rows are padded (SEP, score 0, row 0) and its hypotheses frozen; the loop still runs its max_len - 1 steps, with
 * no host decision.  repetition_penalty (model.py:522-531) rewrites the logits of the columns in a row's prefix before the
 * log-softmax; with constraints attached, banned columns are -inf first.  A prompt's forced steps finish nothing.
 *   num_keep_best        1 .. k: hypotheses kept and returned per clip
 *   length_penalty       the exponent above (finite)
 *   per_node_beam_size   0 = k; else 2 .. k, and k * per_node_beam_size <= 16 (with 1 a SEP candidate would leave a clip short of k
 *                        live beams, which the reference asserts against, model.py:606; so the attachment needs k >= 2)
 *   repetition_penalty   > 0 and finite, 1 = off
 *   scores_out           device fp32 [B][num_keep_best]: the scores, best first; a rank without a hypothesis holds -1e5
 *   lengths_out          device int32 [B][num_keep_best], nullable: tokens of each hypothesis, CLS included, SEP not; 0 = none
 * While it is attached ids_out of the consuming call is [B][num_keep_best][max_len]: rank 0 first, every row filled with SEP
 * behind its hypothesis.  A ONE-SHOT attachment: the next call of the beam family consumes it, whether that call succeeds or is
 * refused; every greedy, draft, score and attention entry point consumes it and fails with GITCAP_ERR_ARG; NULL detaches.  It
 * combines with the frame-count, constraint and prompt attachments.  The options are copied at the attach; the two pointers are
 * written by the consuming call on its stream.  The first consuming call adds the hypothesis store to the beam workspace
 * (gitcap_student_workspace_bytes); a handle that never attaches allocates nothing and makes the launches it made.
 * Errors, GITCAP_ERR_ARG: a field outside the ranges above that do not depend on k, a null or misaligned scores_out, a misaligned
 * lengths_out; at the consuming call num_keep_best > k, per_node_beam_size > k or 1 (k = 1 included), k * per_node_beam_size > 16,
 * and under constraints n_suppress + max_len + k * per_node_beam_size > vocab_size.  Nothing is launched then. */
typedef struct gitcap_student_search_options {
    int32_t num_keep_best;
    float length_penalty;
    int32_t per_node_beam_size;
    float repetition_penalty;
    float* scores_out;
    int32_t* lengths_out;
} gitcap_student_search_options;
int gitcap_student_attach_search(gitcap_student_t* h, const gitcap_student_search_options* o);
/* gitcap_workspace_bytes for this handle: the device bytes of its workspace, attachments' buffers and the stream pool (weights, the
 * window's ring and page-locked memory not counted).  What an attachment's first use adds shows here. */
int gitcap_student_workspace_bytes(const gitcap_student_t* h, int64_t* bytes);
/* test hooks of the two kernels behind it, on caller-owned device buffers.  prompt_stage: ids [rows][ld] row r = cls, tokens
 * 1 .. len - 1 of prompt_ids [rows / k][ld_prompt] row r / k, cls behind them, len = lengths[r / k] clamped to [1, max_len] (max_len <=
 * ld_prompt, max_len <= ld); lp (nullable, fp32 [rows][ld_lp]): columns 0 .. pmin - 2 = 0.0f (1 <= pmin <= ld_lp + 1).
 * student_beam_step: candidates [B][k] (flat index = beam * V + token, best first) -> ids_next rows (prefix 0 .. t of the source row
 * of ids_cur [B * k][ld], the token at t + 1), scores, src_rows; prompt_ids NULL: the plain kernel; else (lengths required,
 * prompt_max_len <= ld_prompt) the forced form where t + 1 < prompt_max_len: a clip with t + 1 < lengths[b] appends
 * prompt_ids[b][t + 1] to every row's own prefix, src_rows the identity, scores and candidates untouched. */
int gitcap_dbg_student_prompt_stage(const int64_t* prompt_ids, int ld_prompt, const int32_t* lengths, int rows, int k, int max_len, int64_t cls,
                                    int64_t* ids, int ld, float* lp, int ld_lp, int pmin, void* stream);
int gitcap_dbg_student_beam_step(const float* cand_scores, const int32_t* cand_idx, const int64_t* ids_cur, int64_t* ids_next, float* scores,
                                 int32_t* src_rows, int B, int k, int V, int t, int ld, const int64_t* prompt_ids, int ld_prompt,
                                 const int32_t* lengths, int prompt_max_len, void* stream);
/* gitcap_score over the student decoder's teacher-forced pass (the rows of gitcap_student_forward_decoder, after
 * gitcap_student_set_memory with `rows` rows): same semantics, outputs and ignore rules; no `beams` (candidates of one clip are
 * rows whose memory the caller repeated).  Checks: gitcap_student_forward_decoder's, plus T < 2, ld_ids < T, ld_lp < T - 1. */
int gitcap_student_score(gitcap_student_t* h, const int64_t* ids, int ld_ids, int rows, int T, const int32_t* lengths, int64_t ignore_id,
                         float* token_lp, int ld_lp, float* row_sum, int32_t* row_cnt, int64_t* top1_ids, float* top1_lp, void* stream);
int gitcap_student_dbg_score_target_logits(gitcap_student_t* h, float* out, int n, void* stream);
/* Per-token attention over the frames, for this handle.  The student's memory is one token per frame, so its cross-attention IS the
 * per-frame attribution: a teacher-forced pass over `ids` against the memory set last -- the rows of gitcap_student_score, without
 * the vocabulary head -- during which one small launch per layer writes the probabilities of the cross-attention (the q and memory
 * K the attention launch reads, its own arithmetic), then their mean over the heads and over all layers (layer = -1) or one, in a
 * fixed order.  frame_mass: device fp32 [rows][T][ld_f], column f = the mass on memory token f (each position's columns sum to 1),
 * ld_f >= mem_tokens; position j is the one whose head predicts ids[r][j + 1]; lengths (nullable, device int32 [rows]): positions
 * j >= lengths[r] are zeros.  Checks: gitcap_student_forward_decoder's, plus T < 1, ld_ids < T, ld_f < mem_tokens, a layer outside
 * [-1, layers).  The first call allocates the probabilities' scratch; every other call of the handle runs the launches it ran. */
int gitcap_student_attention(gitcap_student_t* h, const int64_t* ids, int ld_ids, int rows, int T, int layer, const int32_t* lengths,
                             float* frame_mass, int ld_f, void* stream);
/* The same read-out without a handle: q bf16 [rows * T][H * hd], memory keys k bf16 [rows][F][ldkv] (head h at columns h * hd) ->
 * probs fp32 [rows * T][H][F] = softmax(q . k / sqrt(hd)) and frame_mass [rows][T][ld_f], their head mean.  F <= 64, hd % 8 == 0,
 * hd <= 128, ldkv % 8 == 0. */
int gitcap_dbg_cross_probs(const void* q, const void* k, int ldkv, int rows, int T, int H, int hd, int F, const int32_t* lengths, float* probs,
                           float* frame_mass, int ld_f, void* stream);
/* Its variable-length form: k is PACKED, row r's keys are rows key_off[r] .. key_off[r] + key_len[r] - 1 of it (device int32 [rows]
 * each, 1 <= key_len <= F).  probs stays [rows * T][H][F]: columns from key_len[r] on hold 0, the others the bits of
 * gitcap_dbg_cross_probs at F = key_len[r] on that row's keys.  Synchronises `stream` (the tables are checked on the host first). */
int gitcap_dbg_cross_probs_varlen(const void* q, const void* k, int ldkv, int rows, int T, int H, int hd, int F, const int32_t* lengths, float* probs,
                                  float* frame_mass, int ld_f, const int32_t* key_off, const int32_t* key_len, void* stream);

/* Clips of different length on the student: gitcap_attach_frame_counts for this handle.  The decoder has no positional or temporal
 * term on its memory (model.py:102 and :130-131 are commented out), so a clip of any number of frames is a well-defined input: its
 * cross-attention runs over its own frames and nothing else.
 *   counts  host int32 [B], 1 <= counts[b] <= mem_tokens, B <= max_rows; copied.  NULL detaches.
 * One-shot: consumed by the next of gitcap_student_set_memory, gitcap_student_greedy, gitcap_student_beam_search and
 * gitcap_student_greedy_draft (success or failure), whose B must be the counts' and whose `memory` is then PACKED: device fp32
 * [sum(counts)][d_model], clip-major, no padding.  Exactly sum(counts) rows are cast and projected; the k beams of a clip share its
 * rows (nothing is repeated).  The layout belongs to the memory set: gitcap_student_forward_decoder, _score, _attention and the student
 * rows of gitcap_distill follow it until the next memory is set.  Every clip's results are bit for bit those of the clip run alone on
 * a handle created with mem_tokens = counts[b]; counts that all equal mem_tokens run the dense call, launch for launch.
 * gitcap_student_attention keeps ld_f >= mem_tokens; the columns from a clip's count on hold 0.  The captured token loops read the
 * counts from two device tables at replay: one graph per (B, max_len, ...) serves every set of counts.
 * The gitcap_student_window_* calls do not take counts: with counts attached they fail with GITCAP_ERR_ARG and a message that
 * names the attachment, which they consume.
 * Errors: GITCAP_ERR_ARG for a null handle, B outside [1, max_rows], a count outside [1, mem_tokens] (the message names the clip),
 * and at the consuming call for a B that is not the counts'. */
int gitcap_student_attach_frame_counts(gitcap_student_t* h, const int32_t* counts, int B);
/* gitcap_student_window_greedy before the window is full: captions the n tokens pushed since the reset (1 <= n; n >= mem_tokens is
 * gitcap_student_window_greedy itself), so a live stream shows a caption from its first admitted frame on.  All clips of a window
 * share n.  Bit for bit gitcap_student_greedy on those n tokens per clip with counts = n attached.  frames_out (host int32,
 * nullable) = the tokens the caption saw, min(n, mem_tokens).  Takes the log-probability and top-k attachments as
 * gitcap_student_window_greedy does.  The beam and draft window calls have no partial form: they need a full window.
 * GITCAP_ERR_STATE when nothing has been pushed since the reset. */
int gitcap_student_window_greedy_partial(gitcap_student_t* h, int max_len, int stop, int64_t* ids_out, int32_t* steps_out, int32_t* frames_out,
                                         void* stream);

/* Stream pool: the memory-token window for several cameras on one handle.  The window above is ONE ring cursor: its clips advance
 * in lockstep.  Cameras that start at different times, behind gates that admit different frames, are each at their own fill level
 * and ring position; the pool keeps S independent windows (streams), takes tokens for any of them in any mix, and captions any
 * subset of them as one ragged batch.  A token's K | V rows are computed once, at the push (the GEMM of gitcap_student_window_push
 * over the n packed rows: a K | V row has the same bits whichever launch computed it, at every number of rows); a pool call copies
 * each named stream's rows, oldest first, PACKED, to where gitcap_student_set_memory would have written them for clips of those
 * lengths, writes the key tables of gitcap_student_attach_frame_counts and runs the token loop of the full call (its captured
 * graphs, which read the tables at replay).  No host decision lies between the copy and the token loop.
 * Contract: row r of gitcap_student_pool_greedy is bit for bit row r of gitcap_student_greedy with the streams' token counts attached
 * (gitcap_student_attach_frame_counts) on the streams' current tokens, oldest first -- ids, log-probabilities and alternatives --
 * and, as there, what the row would be alone.  When every named stream holds mem_tokens tokens the layout is the dense one and the
 * call takes the dense launches, as gitcap_student_window_greedy on a full window does.
 *   reset   n_streams = S, 1 <= S <= 4096: allocates (or, for the S of the last reset, reuses) the ring, bf16
 *           [num_layers][S][mem_tokens][2 d_model], the staging of one push (max_rows * mem_tokens rows: the tokens cast to bf16, their
 *           K | V rows of every layer, the slot table) and the table of one call; empties every stream.  S = 0 releases all of it;
 *           so do gitcap_student_finalize (the rows came from the weights it replaces) and destroy.  A set-up step: a change of S
 *           waits for the device.  A handle that never resets a pool allocates nothing and runs exactly the launches it ran before.
 *           The pool is state of its own: gitcap_student_window_reset / _push / _greedy* neither read nor change it, nor the pool
 *           calls the window.
 *   push    memory: device fp32 [n][d_model], n tokens; stream_ids: HOST int32 [n], token i goes to stream stream_ids[i] behind
 *           that stream's earlier tokens, this push's earlier ones included.  1 <= n <= max_rows * mem_tokens (the staging), and a
 *           stream gets at most mem_tokens tokens in one push (more would write one ring slot twice in one launch: push twice).
 *           The ids are checked on the host before anything is enqueued; a refused push changes nothing.  Work: one cast, one
 *           K | V GEMM per layer over the n rows, one scatter launch for all layers.  Like a window push it writes neither the
 *           decoder's memory nor the self-attention cache.
 *   greedy  stream_ids: HOST int32 [B], 1 <= B <= max_rows, distinct; decoder row r is stream stream_ids[r], in the caller's order,
 *           and sees its last n_r = min(tokens pushed, mem_tokens) tokens.  frames_out (host int32 [B], nullable) = n_r.  The other
 *           arguments, the stop rule and the ids_out / steps_out layout as gitcap_student_greedy.  Takes the attachments of
 *           gitcap_student_attach_token_logprobs and gitcap_student_attach_top_logprobs as gitcap_student_window_greedy does;
 *           attached frame counts are refused (and consumed) with the window calls' message.  Leaves the handle as
 *           gitcap_student_greedy with those counts would.  There is no draft form of the pool call.
 *   beam    gitcap_student_pool_beam_search: the beam form of the pool call, k beams per named stream (B * k <= max_rows, k <= 16).
 *           The streams' K|V rows are copied packed, once per stream, and the k rows of stream r read them through the key tables
 *           (gitcap_student_attach_frame_counts' scheme for beams: nothing is repeated), so row r is bit for bit row r of
 *           gitcap_student_beam_search with the streams' token counts attached.  ids_out as gitcap_student_beam_search; takes the
 *           constraint, prompt and search attachments (gitcap_student_attach_search) as that call does; stream_ids / B are checked
 *           as by the greedy form, with its errors.  Leaves the handle with B * k rows.
 *   drop    empties one stream (a camera that reconnected); the others are untouched.
 *   counts  host int32 [S]: the tokens each stream holds, 0 .. mem_tokens.
 * Pushes and pool calls may be issued on different streams: two events of the pool's own order a push behind the last pool call's
 * copy and the last push, and a pool call behind the last push.  The two page-locked tables are reused behind an event each.
 * Errors: GITCAP_ERR_ARG for a null handle or pointer, n_streams outside [0, 4096], n outside [1, max_rows * mem_tokens], a stream
 * id outside [0, S), more than mem_tokens tokens for one stream in one push, B outside [1, max_rows], a stream named twice in a call,
 * attached frame counts, and the length / stop-rule / attachment checks of gitcap_student_greedy; GITCAP_ERR_STATE for a call
 * before any reset (or after the pool was released), a named stream that holds no token (nothing is launched), and weights not
 * finalized.  gitcap_abi_version is unchanged: these are new symbols only. */
int gitcap_student_pool_reset(gitcap_student_t* h, int n_streams);
int gitcap_student_pool_push(gitcap_student_t* h, const float* memory, const int32_t* stream_ids, int n, void* stream);
int gitcap_student_pool_greedy(gitcap_student_t* h, const int32_t* stream_ids, int B, int max_len, int stop, int64_t* ids_out,
                               int32_t* steps_out, int32_t* frames_out, void* stream);
int gitcap_student_pool_beam_search(gitcap_student_t* h, const int32_t* stream_ids, int B, int k, int max_len, int64_t* ids_out, void* stream);
int gitcap_student_pool_drop(gitcap_student_t* h, int stream_id);
int gitcap_student_pool_counts(const gitcap_student_t* h, int32_t* counts_out);

/* Teacher-student divergence of given captions, forward only: KL(teacher || student) of every position's next-token distribution
 * at a temperature -- LOSS 2 of DistillationTrainer.training_step (src/models/model.py:919-935: KLDivLoss('batchmean') of
 * log_softmax(student / t) against softmax(teacher / t)) -- without either model's [rows * T][V] logits: both vocabulary heads run
 * over the same 16-column tiles in one launch that keeps seven per-tile statistics, and one merge launch follows (csrc/skinny.hip:
 * skinny_head_dual_kernel, csrc/select.hip: distill_final_kernel).
 * Preconditions: gitcap_score's on the teacher (after gitcap_encode / gitcap_set_visual; rows = encoded clips * beams) and
 * gitcap_student_score's on the student (after gitcap_student_set_memory with `rows` rows, a clip's rows repeating its memory);
 * both handles on one device, equal vocab_size, widths (768 | 1024, 576) or (128, 64), temperature > 0 and finite, T >= 1,
 * ld_ids >= T, out and out->kl non-null, ld_kl >= T, ld_lp >= T - 1 where a log-probability output is set.  Every refusal is
 * GITCAP_ERR_ARG / GITCAP_ERR_STATE with the message on the TEACHER's last_error, and launches nothing.
 * Both passes run on `stream` (teacher, then student), synchronous path, slot 0; the text K/V of positions 0 .. T - 1 of both
 * handles are overwritten, as gitcap_score does.  Outputs (device; all but kl nullable), with t = teacher logit / temperature:
 *   kl            fp32 [rows][ld_kl], positions 0 .. T - 1: sum_v softmax(t)_v (log_softmax(t)_v - log_softmax(s)_v) in nats (NOT times
 *                 temperature^2); +inf where the teacher gives mass to a word whose student logit is -inf; 0 at a position
 *                 j >= lengths[r] (lengths nullable, device int32 [rows]) and for a row whose teacher logits are all -inf
 *   teacher_top1 / student_top1  int64 [rows][T]: each model's arg-max under the token loops' tie rule; agree uint8 [rows][T]
 *   teacher_lp / student_lp      fp32 [rows][ld_lp], positions 0 .. T - 2: log-probability (at the temperature) of the given next
 *                 token ids[r][j + 1] under gitcap_score's ignore rules (0 where ignored); temperature 1: gitcap_score's bits
 *   row_kl_sum fp32 [rows] / row_cnt int32 [rows]: the counted positions' kl added in ascending order, and their number
 * A row's values are bit for bit independent of the rows beside it.  The first call allocates the partial buffers on the teacher
 * handle; gitcap_workspace_bytes counts them from then on.  Handles that never call it run the launches they ran before. */
typedef struct gitcap_distill_out {
    float* kl; int ld_kl;
    int64_t* teacher_top1; int64_t* student_top1; uint8_t* agree;
    float* teacher_lp; float* student_lp; int ld_lp;
    float* row_kl_sum; int32_t* row_cnt;
} gitcap_distill_out;
int gitcap_distill(gitcap_t* teacher, gitcap_student_t* student, const int64_t* ids, int ld_ids, int rows, int beams, int T,
                   const int32_t* lengths, int64_t ignore_id, float temperature, const gitcap_distill_out* out, void* stream);
/* debug: the dual head on caller-owned buffers.  Xt [M][ldxt] / Xs [M][ldxs] bf16 rows, Wt [Npad16][Kt] (bf16, or e4m3 codes with
 * wscale [Npad16]) / Ws [Npad16][Ks] bf16, biases [N] (nullable); seven partials [M][ntiles]; targets int64 [M] (nullable; one
 * column per row) -> t_logit / s_logit fp32 [M] (untouched for a target outside [0, N)). */
int gitcap_dbg_vocab_head_dual(const void* Xt, int ldxt, const void* Wt, const float* wscale, const float* bias_t, int Kt, const void* Xs,
                               int ldxs, const void* Ws, const float* bias_s, int Ks, int M, int N, float inv_temperature, float* t_max,
                               int32_t* t_idx, float* t_sum, float* s_max, int32_t* s_idx, float* s_sum, float* cross,
                               const int64_t* targets, float* t_logit, float* s_logit, void* stream);
/* debug: the merge of gitcap_distill on caller-owned buffers: partials [rows * T][ntiles], t_logit / s_logit [rows * T] (required
 * with the matching log-probability output), ids [rows][ld_ids]; out as gitcap_distill's, out->kl required. */
int gitcap_dbg_distill_final(const float* t_max, const int32_t* t_idx, const float* t_sum, const float* s_max, const int32_t* s_idx,
                             const float* s_sum, const float* cross, int ntiles, const float* t_logit, const float* s_logit,
                             const int64_t* ids, int ld_ids, int rows, int T, const int32_t* lengths, int64_t ignore_id, int V,
                             const gitcap_distill_out* out, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * Student image encoder (SURVEY.md par. 8 row f.2): timm's TinyVit as StudentCandidateV1 loads it with
 * features_only=True (src/models/model.py:35-47, :108-126) -- conv stem, MBConv stage 0, three stages of
 * PatchMerging + windowed-attention blocks -- on bf16 activations (csrc/tinyvit.hip; rounding points in DESIGN.md).
 * Tensor names are the canonical checkpoint keys without the image_encoder.model. prefix (patch_embed.conv1.*,
 * stages_{i}.blocks.{j}.attn.qkv.weight, ...), with every Conv2d + BatchNorm2d pair folded by the caller into
 * <prefix>.weight / <prefix>.bias.  Same ownership, error and threading rules as the gitcap_student_* entry points.
 * ------------------------------------------------------------------------------------------------- */
typedef struct gitcap_tinyvit gitcap_tinyvit_t;
struct gitcap_tinyvit_config {
    int32_t img_size, embed_dims[4], depths[4], num_heads[4], window_sizes[4],
            merge_strides[4] /* [0] unused */, max_frames;
    float ln_eps;                                    /* 1e-5 */
};
/* refuses, before touching the device, head_dim != 32, widths not multiples of 32, stage maps not divisible by their
 * windows, windows above 14 and merge strides other than 1 or 2 */
int gitcap_tinyvit_create(const struct gitcap_tinyvit_config* cfg, int device, gitcap_tinyvit_t** out);
void gitcap_tinyvit_destroy(gitcap_tinyvit_t* h);
const char* gitcap_tinyvit_last_error(const gitcap_tinyvit_t* h);
/* host fp32 data, logical shape (conv weights [Cout][Cin/groups][k][k]); GEMM weights are stored as bf16 */
int gitcap_tinyvit_load_tensor(gitcap_tinyvit_t* h, const char* name, const float* data, const int64_t* shape, int rank);
int gitcap_tinyvit_finalize(gitcap_tinyvit_t* h);
/* frames: device fp32 [n][3][img][img] (normalised, as model.py:117 receives them) -> memory device fp32 [n][C3] (the mean
 * of the stage-3 map, model.py:124); fmaps: nullable array of 4 nullable device fp32 NCHW outputs [n][Ci][Hi][Wi].
 * n <= max_frames. */
int gitcap_tinyvit_encode(gitcap_tinyvit_t* h, const float* frames, int n, float* memory, float* const* fmaps, void* stream);
/* The same from camera frames: frames_hwc_bgr device uint8 [n][H][W][3] (OpenCV layout, src/real_time_inference.py:39), the input
 * of gitcap_preprocess.  Replaces the reference's per-frame host transform (real_time_inference.py:16-28: ToTensor, bicubic
 * Resize of the shorter side to img_size, CenterCrop(img_size), BGR -> RGB, CLIP Normalize) AND the gather of the first stem
 * convolution: one kernel writes the convolution's bf16 im2col rows straight from the uint8 frames, no fp32 frame tensor exists.
 * Contract: memory and all four fmaps equal, bit for bit, gitcap_preprocess(crop = img_size) followed by gitcap_tinyvit_encode.
 * GITCAP_ERR_ARG: null handle / frames / memory, n < 1, n > max_frames, H or W < 1 or a size whose resized frame is smaller
 * than img_size.  No workspace beyond gitcap_tinyvit_encode's. */
int gitcap_tinyvit_encode_raw(gitcap_tinyvit_t* h, const uint8_t* frames_hwc_bgr, int n, int H, int W, float* memory,
                              float* const* fmaps, void* stream);

/* ---- scene-change gate for live frames (gitcap/framegate.py) -------------------------------------------------------------
 * Replaces: the distances of frame_mse_difference_sampling / scene_change_detection_sampling
 *                                                         src/utils/frame_sampling_methods.py:201-297
 * How far B camera frames are from B reference frames (the last frames a caller kept), computed on the device in one pass over
 * both: frames_hwc_bgr, ref_hwc_bgr device uint8 [B][H][W][3] (the layout of gitcap_tinyvit_encode_raw / gitcap_window_push_raw;
 * any alignment).  All five outputs are device memory, each may be NULL:
 *   ssd[B]              exact sum over the H*W*3 bytes of (frame - ref)^2, in integers (not the reference's uint8 arithmetic,
 *                       which wraps modulo 256, :237)
 *   hist_frame[B][256]  exact counts of the byte values of channel `channel` (0, 1 or 2 of the BGR triple; the reference
 *   hist_ref[B][256]    histograms the red channel, :282-286, which is 2 here) of the frame / of the reference frame
 *   mse[B]              (double)ssd / (H*W*3)
 *   chisq[B]            sum over the bins i with hist_ref[i] > 0, in ascending i, of (hist_ref[i] - hist_frame[i])^2 / hist_ref[i]
 *                       in fp64: OpenCV's HISTCMP_CHISQR with the reference frame as H1 (:284-288)
 * Stateless (no handle): the partial sums live in a stream-ordered allocation of the call, so calls on different streams share
 * nothing.  GITCAP_ERR_ARG: a null input, B, H or W < 1, channel outside 0..2, H*W*3 >= 2^31 or B >= 65536. */
int gitcap_frame_change(const uint8_t* frames_hwc_bgr, const uint8_t* ref_hwc_bgr, int B, int H, int W, int channel,
                        uint64_t* ssd, uint32_t* hist_frame, uint32_t* hist_ref, double* mse, double* chisq, void* stream);

/* ---- frame sampling of whole videos (gitcap/sampling.py; csrc/framesample.hip) ----------------------------------------------
 * Replaces: frame_mse_difference_sampling, scene_change_detection_sampling, clustered_sampling
 *                                                         src/utils/frame_sampling_methods.py:135-297
 * A decoded video is device uint8 [N][H][W][3] (BGR, any alignment).  The calls below choose its frames without a host decision:
 * every step of a call is enqueued at once on `stream`, the steps are ordered by the stream alone (no kernel waits on another
 * workgroup), and what a step needs from the one before -- the chain's reference frame, whether k-means has converged -- is a word
 * in a stream-ordered allocation of the call.  Handle-free; nothing is synchronised.  Every call returns GITCAP_ERR_ARG before any
 * launch for a null pointer (where not stated otherwise) or N <= 0, and for what its own paragraph lists.
 *
 * gitcap_frame_chain: the reference's two sequential samplers over a whole video.  Every `every`-th frame is looked at (frame 0
 * included, as gitcap.framegate.FrameGate).  Frame 0 is kept.  A later looked-at frame i is compared with the last frame kept:
 * dist[i] is, bit for bit, the mse (metric 0) or chisq (metric 1, channel `channel` of the BGR triple) gitcap_frame_change gives
 * for that pair, keep[i] = dist[i] > threshold.  dist of frame 0 and of frames not looked at is NaN, their keep 0 (frame 0: 1).
 * The two differences from the reference's arithmetic are gitcap_frame_change's (exact integer MSE, one channel order).
 * GITCAP_ERR_ARG: H or W < 1, H*W*3 >= 2^31, metric outside 0..1, channel outside 0..2, every < 1. */
int gitcap_frame_chain(const uint8_t* video_hwc_bgr, int N, int H, int W, int metric, int channel, double threshold, int every,
                       uint8_t* keep, double* dist, void* stream);

/* X[N][h2*w2*3] (fp32, element order y, x, channel): every frame resized to h2 x w2 by bilinear interpolation with half-pixel
 * centres -- output row y samples source row ((2y + 1) H / h2 - 1) / 2, not below 0, the row beyond the last repeats it; columns
 * alike.  Taps and weights come from integer quotients, the blend a w00 + b w01 + c w10 + d w11 is fp32, and nothing is rounded
 * back to uint8 (the reference's cv2.resize works in fixed point and does; not reproduced).
 * GITCAP_ERR_ARG: H, W, h2 or w2 < 1, h2 or w2 > 2^22. */
int gitcap_frame_features(const uint8_t* video_hwc_bgr, int N, int H, int W, int h2, int w2, float* X, void* stream);

/* Lloyd's algorithm on the rows of X[N][D] (fp32) with k clusters; the centroids start at the rows init_idx[k] (device int32; an
 * index outside [0, N) is clamped).  An iteration assigns, then updates:
 *   assign   labels[n] = arg min over c of sum_d (X[n][d] - centroids[c][d])^2, the direct difference in fp32 in a fixed order;
 *            ties go to the lower c
 *   update   centroids[c] = the mean of the rows labelled c, added in ascending n in fp32 (no atomics on floats: two runs are
 *            bit-identical); a cluster without rows keeps its centroid (sklearn relocates it)
 * All max_iter iterations are enqueued.  The first iteration whose assign changes no label is the last: its update and everything
 * behind it return at once, and iters[0] is that iteration's number (max_iter if there is none).  labels[N], centroids[k][D] and
 * iters[1] are device memory.  GITCAP_ERR_ARG: D < 1, k < 1, k > N, k > 65535, max_iter outside [1, 2^20]. */
int gitcap_kmeans(const float* X, int N, int D, int k, const int32_t* init_idx, int max_iter, int32_t* labels, float* centroids,
                  int32_t* iters, void* stream);
/* One assign step alone: labels[N] in (any value; -1 = none) and out, changed[0] += the number of labels that changed. */
int gitcap_dbg_kmeans_assign(const float* X, int N, int D, int k, const float* centroids, int32_t* labels, int32_t* changed, void* stream);
/* One update step alone: centroids[k][D] in and out (a cluster without rows keeps its row). */
int gitcap_dbg_kmeans_update(const float* X, int N, int D, int k, const int32_t* labels, float* centroids, void* stream);

/* The kept frames' indices in ascending order: idx[0 .. count[0]), idx[count[0] .. N) = -1.  keep[N] non-null: frame i is kept iff
 * keep[i] != 0; else labels[N]: frame 0 and every i with labels[i] != labels[i-1] (the reference's run-boundary rule, :186-192).
 * With K kept frames and K > max_frames, the selection is thinned to kept[floor(j K / max_frames)], j = 0 .. max_frames - 1
 * (a model's temporal embedding has a frame limit).  One workgroup.  GITCAP_ERR_ARG: keep and labels both null, max_frames < 1. */
int gitcap_frame_select(const uint8_t* keep, const int32_t* labels, int N, int max_frames, int64_t* idx, int32_t* count, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GITCAP_H */
