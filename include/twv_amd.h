/* twv_amd.h -- C-ABI of the MI355X (gfx950) WaveNet-vocoder hot path.
 *
 * Drop-in boundary for hccho2/Tacotron-Wavenet-Vocoder-Korean's WaveNet generation path.  The reference has
 * no FFI of its own: the path sits behind Python callables on a TensorFlow session.
 * Each entry point below names the reference callable it replaces (file:line in /root/reference); the
 * Python host in tacotron-wavenet-vocoder-korean_amd/ binds them with ctypes (INTEGRATION.md shows the stub).
 *
 * Conventions: plain C, raw DEVICE pointers + explicit sizes, no framework types.  Every buffer is owned by
 * the caller; the handle owns host-side metadata only.  `stream` is a hipStream_t passed as void* (NULL =
 * default stream).  All calls are asynchronous on `stream` unless stated.  Return 0 = TWV_OK, else a TWV_E_*
 * code with text in twv_last_error() (thread-local).  One handle per GPU; thread-compatible, not thread-safe.
 */
#ifndef TWV_AMD_H
#define TWV_AMD_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define TWV_MAX_LAYERS 64

enum { TWV_OK = 0, TWV_E_INVALID = 1, TWV_E_UNSUPPORTED = 2, TWV_E_HIP = 3, TWV_E_KERNEL = 4,
       TWV_E_BUSY = 5 /* a persistent kernel found the device occupied by other work: nothing was done, retry later */ };

/* WaveNetModel constructor arguments (wavenet/model.py:8-10) + hparams.upsample_factor (hparams.py:79) */
typedef struct {
    int32_t n_layers;
    int32_t dilations[TWV_MAX_LAYERS];   /* hparams.dilations */
    int32_t residual_channels;           /* R: 32, 64 or 128 */
    int32_t dilation_channels;           /* D: 32, 64 or 128 (independent of R) */
    int32_t skip_channels;               /* S, multiple of 64, <= 1024 */
    int32_t quantization_channels;       /* Q */
    int32_t out_channels;                /* MoL parameter count (3*nr_mix <= 63); ignored when !scalar_input */
    int32_t scalar_input;                /* 1: raw/mulaw scalar input + MoL output; 0: one-hot input + Q-way softmax */
    int32_t initial_filter_width;        /* <= 64 */
    int32_t use_biases;
    int32_t gc_channels;                 /* 0 = no global conditioning, else <= 64 */
    int32_t gc_cardinality;              /* 0 with gc_channels > 0: no gc_embedding table; every `gc_ids` argument then points at (B, gc_channels)
                                            float embeddings instead of int32 ids (_embed_gc's second branch, model.py:199-207) */
    int32_t lc_channels;                 /* num_mels; 0 = no local conditioning, else <= 128 */
    int32_t n_upsample;                  /* len(upsample_factor) <= 4 */
    int32_t upsample_factor[4];
} twv_wavenet_dims;

typedef struct twv_wavenet twv_wavenet;   /* opaque, host-side */

const char* twv_last_error(void);
const char* twv_version(void);

/* WaveNetModel.__init__ (model.py:8-30): validates the dims, computes layouts.  No device memory is touched. */
int twv_wavenet_create(const twv_wavenet_dims* dims, twv_wavenet** out);
void twv_wavenet_destroy(twv_wavenet* h);

/* WaveNetModel.calculate_receptive_field (model.py:31-39) */
int twv_wavenet_receptive_field(const twv_wavenet* h);
int twv_wavenet_hop_size(const twv_wavenet* h);              /* prod(upsample_factor) */

/* sizes (bytes unless noted) of the caller-owned device buffers */
size_t twv_wavenet_blob_floats(const twv_wavenet* h);        /* canonical checkpoint blob, in floats */
size_t twv_wavenet_packed_bytes(const twv_wavenet* h);       /* streaming-layout weights */
size_t twv_wavenet_state_bytes(const twv_wavenet* h, int batch);              /* delay lines etc. (model.py:49-64) */
size_t twv_wavenet_cond_bytes(const twv_wavenet* h, int batch, int n_steps);  /* hoisted lc/gc projections */

/* tf.train.Saver.restore equivalent (generate.py:157-161): re-lays the canonical blob (checkpoint tensors,
 * TF layouts, order of DESIGN.md) into the streaming layout.  blob and packed are device pointers. */
int twv_wavenet_pack(const twv_wavenet* h, const float* blob, void* packed, void* stream);

/* net.queue_initializer (model.py:64, generate.py:163): zero every delay line of every stream. */
int twv_wavenet_reset_state(const twv_wavenet* h, void* state, int batch, void* stream);

/* The same for the streams b with flags[b] != 0 alone (flags: DEVICE int32 (batch)): stream b's part of `state` -- causal queue,
 * previous lc frame, delay lines and their positions, of every workgroup that serves the stream -- becomes what
 * twv_wavenet_reset_state leaves; every other stream's state stays bit for bit.  One launch, no host synchronisation.  Right for
 * every state layout twv_wavenet_state_bytes selects (generic kernel at any "groups", both XCD kernels, the wide kernel); the
 * exchange areas behind the per-stream blocks are per launch (zeroed by every generate / prime call) and are not touched. */
int twv_wavenet_reset_streams(const twv_wavenet* h, void* state, int batch, const int32_t* flags, void* stream);

/* Utterance queue (DESIGN.md "Utterance queue"): a list of utterances of any lengths on `batch` stream slots, refilled at chunk
 * boundaries.  table: DEVICE int32 (n_chunks, batch, 4) = {utterance index or -1 for an idle slot, first frame of the piece, valid
 * frames (<= chunk_frames), 1 where the utterance starts in this chunk}; frame_off: DEVICE int64 (n_utterances + 1) prefix sums of
 * the lengths in mel frames.  Packed inputs, utterances back to back: mels (sum frames, lc) float32; uniforms (sum frames * hop,
 * nr_mix + 1) float32 or (sum frames * hop) float64 (one-hot); seeds (n_utterances) float32 | int32; gc_ids (n_utterances) int32
 * or NULL.
 *   twv_wavenet_queue_stage   writes chunk `chunk`'s inputs: mel_chunk (batch, chunk_frames, lc), zeros past an utterance's end
 *                             and in idle slots; u_chunk (batch, chunk_frames * hop, ...), 0.5 there; gc_chunk (batch) (0 when
 *                             idle; NULL allowed); first_input (batch): the utterance's seed where it starts here, else the last
 *                             sample of prev_out (batch, chunk_frames * hop), the previous chunk's output, read on the device
 *                             (NULL for chunk 0); reset_flags (batch) for twv_wavenet_reset_streams.
 *   twv_wavenet_queue_collect copies every slot's valid prefix of out_chunk (batch, chunk_frames * hop) into result, the packed
 *                             (sum frames * hop) float32 samples | int32 class ids.
 * Per chunk: stage, reset_streams, condition(_mel), generate for chunk_frames * hop steps, collect. */
int twv_wavenet_queue_stage(const twv_wavenet* h, const int32_t* table, int chunk, int batch, int chunk_frames,
                            const int64_t* frame_off, const float* mels, const void* uniforms, const void* seeds,
                            const int32_t* gc_ids, const void* prev_out, float* mel_chunk, void* u_chunk, int32_t* gc_chunk,
                            void* first_input, int32_t* reset_flags, void* stream);
int twv_wavenet_queue_collect(const twv_wavenet* h, const int32_t* table, int chunk, int batch, int chunk_frames,
                              const int64_t* frame_off, const void* out_chunk, void* result, void* stream);

/* WaveNetModel.create_upsample (model.py:102-111): mel (B, T_mel, lc) -> out (B, T_mel*hop, lc).
 * scratch: device buffer of at least the output size (ping-pong for the transposed-conv stages). */
int twv_wavenet_upsample(const twv_wavenet* h, const void* packed, const float* mel, int batch, int t_mel,
                         float* out, float* scratch, void* stream);

/* Hoists the per-step 1x1 projections of _create_dilation_layer (model.py:71-83) out of the sample loop:
 * lc_filter/lc_gate of every layer for all n_steps frames of `upsampled` (B, n_steps, lc), and gc_filter/gc_gate
 * of gc_embedding[gc_ids] (model.py:181-212).  cond is twv_wavenet_cond_bytes(batch, n_steps). */
int twv_wavenet_condition(const twv_wavenet* h, const void* packed, const float* upsampled, const int32_t* gc_ids,
                          int batch, int n_steps, void* cond, void* stream);

/* Fused conditioning: when the XCD-per-stream kernel serves this (handle, batch) -- see the "xcd"
 * option -- create_upsample (model.py:102-111) and the lc projections (model.py:75-83) run INSIDE the generation launch, row by
 * row, ahead of the sample loop: neither the (B, T, lc) upsampled tensor nor a projection table is ever materialised.
 *   twv_wavenet_fused_conditioning : 1 if available for this handle and batch, else 0
 *   twv_wavenet_cond_bytes_mel     : size of `cond` for twv_wavenet_condition_mel
 *   twv_wavenet_condition_mel      : mel (B, t_mel, lc) as generate.py:151 hands it over, gc_ids (B) -> cond; the following
 *                                    twv_wavenet_generate call may run up to t_mel*hop steps (row t = frame pushed at step t).
 * Results are bit-identical to twv_wavenet_upsample + twv_wavenet_condition. */
int twv_wavenet_fused_conditioning(const twv_wavenet* h, int batch);
/* the generation kernel twv_wavenet_generate launches for this (handle, batch, options) on the current device:
 * "wn_xcd_generate_kernel", "wn_xcd_many_kernel" or "wn_generate_kernel" (static string; measurement label, bench.py) */
const char* twv_wavenet_kernel_name(const twv_wavenet* h, int batch);
size_t twv_wavenet_cond_bytes_mel(const twv_wavenet* h, int batch, int t_mel);
int twv_wavenet_condition_mel(const twv_wavenet* h, const void* packed, const float* mel, const int32_t* gc_ids,
                              int batch, int t_mel, void* cond, void* stream);

/* predict_proba_incremental (model.py:215-245) iterated by the generate.py:202-233 host loop, as ONE persistent
 * kernel launch per call: n_steps autoregressive steps for `batch` independent streams.
 *   first_input : (B) the sample fed at step 0 (generate.py:204 waveform[:,-1:]); float32 when scalar_input,
 *                 int32 class ids otherwise.  Later steps feed back the sample just drawn (generate.py:233).
 *   uniforms    : scalar_input: (B, n_steps, nr_mix+1) float32 in [1e-5, 1-1e-5] -- the two tf.random_uniform draws
 *                 of mixture.py:103,110;  one-hot: (B, n_steps) float64 in [0,1) -- np.random.choice's draw
 *                 (generate.py:231).  Injected so that results are reproducible (the reference is unseeded).
 *   temperature : generate.py:219-222 (one-hot only).
 *   out         : (B, n_steps) float32 samples in [-1,1] (scalar_input) or int32 class ids.
 *   status      : device int32[4]; [0] = 0 on success, else an internal code (watchdogs; 31 = NaN class probabilities; checked by twv_wavenet_status).
 * State carries over between calls (n_steps=1 reproduces a single sess.run of generate.py:211).
 * cond must cover the same n_steps as this call (row t = frame pushed at step t).
 *   debug       : optional, (B, debug_steps, NL*(D+R) + Opad) float32, Opad = out channels rounded up to 64: per step and layer the
 *                 gated output z (D floats) then the layer output x (R floats), then the raw network outputs.  NL*64 + Opad at
 *                 R = D = 32.
 * Wide models ((R, D) != (32, 32)) run wn_wide_generate_kernel: one workgroup per stream, no condition on the batch size or on a free
 * device, no watchdog codes (it contains no wait).  Their `cond` is [B][NL][2D] gc projections then [B][n_steps][NL][2D] lc
 * projections (twv_wavenet_cond_bytes says so); twv_wavenet_fused_conditioning is 0 for them. */
int twv_wavenet_generate(const twv_wavenet* h, const void* packed, void* state, const void* cond,
                         const void* first_input, const void* uniforms, double temperature,
                         int batch, int n_steps, void* out, int32_t* status, float* debug, int debug_steps,
                         void* stream);

/* Priming (generate.py:168-180, --wav_seed): feeds `inputs` (B, n_steps; float32 | int32 ids) one per step WITHOUT sampling,
 * exactly like the reference's priming loop that discards next_sample: only the causal queue and the delay lines advance.
 * cond as for twv_wavenet_generate (the reference primes with an all-zero local condition). */
int twv_wavenet_prime(const twv_wavenet* h, const void* packed, void* state, const void* cond, const void* inputs,
                      int batch, int n_steps, int32_t* status, void* stream);

/* synchronises `stream` and converts a non-zero status word into an error: TWV_E_BUSY (the generation kernel's role workgroups could
 * not all become resident because other kernels hold CUs -- the launch did nothing, the state is unchanged, retry), TWV_E_INVALID (the
 * conditioning buffer was built for another kernel selection) or TWV_E_KERNEL (a wait inside the kernel ran out: watchdog code). */
int twv_wavenet_status(const int32_t* status, void* stream);

/* launch geometry knobs (performance only, results are bit-identical): "xcd" = 1 (default): the XCD-per-stream kernel
 * (stream b on XCD b % 8, up to four streams per XCD; every weight register-resident across the XCD's CUs, fused conditioning)
 * whenever the model is the hparams-default MoL shape (scalar input, initial_filter_width 32, skip_channels 512,
 * out_channels <= 32, <= 50 layers: hparams.py's default stack), batch <= 32 (<= 16 with more than 30 layers) and the device has
 * 256 CUs; 0 = always the generic kernel.  Set it (and "groups") BEFORE sizing / resetting the
 * state and conditioning buffers.  "groups" = workgroups per stream of the generic kernel (0 auto; an explicit value also selects
 * the generic kernel), "workers" =
 * worker waves per stream workgroup (4 | 3), "helpers" = 1 (default: conv1d_1 and conv1d_2's chunk partials run in one helper
 * workgroup per stream slice when twice the workgroups are co-resident) | 2 (conv1d_1 only) | 0 (none).
 * "spin_looks" = 1 .. 65535 (default 4096): looks a wait on the XCD kernel's sample-to-sample path takes as a bare spin before its
 * watchdog loop takes over; 1 sends every wait through the watchdog loop after one look (a test aid: same results, slower).
 * On a wide model ((R, D) != (32, 32)) all of these are accepted and have no effect: wn_wide_generate_kernel has one geometry. */
int twv_wavenet_set_option(twv_wavenet* h, const char* name, int value);

/* optional in-kernel phase timestamps (tuning aid): device uint64[steps][80]; per step of stream 0's chain wave:
 * [0] step start, [1] causal layer done, [2] residual stack done, [3..6] the four workgroup barriers (skip sum, conv1d_1,
 * conv1d_2, sample), [7] wall clock (100 MHz), [8+l] layer l done.  Shader-clock ticks (s_memtime).  NULL disables. */
int twv_wavenet_set_profile_buffer(twv_wavenet* h, void* dev_u64, int steps);

/* wavenet/ops.py:22-33 mu_law_encode, ops.py:36-47 mu_law_decode (quantization True / False) */
int twv_mu_law_encode(const float* audio, int64_t n, int quantization_channels, int32_t* out, void* stream);
int twv_mu_law_decode(const int32_t* q, int64_t n, int quantization_channels, float* out, void* stream);
int twv_mu_law_expand(const float* y, int64_t n, int quantization_channels, float* out, void* stream);

/* utils/audio.py:14-17 save_wav's peak normalisation, per row: out = int16(wav * float32(32767 / max(0.01, max|wav|))).
 * wav (rows, n) float, out (rows, n) int16, scratch: rows*64 floats. */
int twv_wav_to_int16(const float* wav, int rows, int64_t n, int16_t* out, float* scratch, void* stream);

/* generate.py:219-231 on rows of logits in device memory: model.py:243 float64 softmax -> float32, the temperature rescale
 * (np.log(p) / T, minus its log-sum-exp, np.exp) and legacy np.random.choice (float64 cumsum / last / searchsorted 'right')
 * with the uniform draw injected.  logits (rows, Q) float, uniforms (rows) double in [0,1), out (rows) int32 class ids,
 * proba (rows, Q) float = generate.py:222's scaled_prediction, or NULL.  The generation kernels draw with the same code.
 * A row whose probabilities are not numbers (a NaN or infinite logit) gets class id -1: np.random.choice raises
 * "ValueError: probabilities contain NaN" on it.  Inside twv_wavenet_generate the same condition sets status code 31, which
 * twv_wavenet_status turns into TWV_E_KERNEL with that explanation. */
int twv_sample_categorical(const float* logits, int64_t rows, int quantization_channels, double temperature, const double* uniforms,
                           int32_t* out, float* proba, void* stream);

/* elementary functions of the arithmetic contract, evaluated on the device (parity tests pin them bit for bit) */
int twv_eval_elementwise(int fn /*0 tanh,1 sigmoid,2 exp,3 log,4 log1p*/, const float* x, int64_t n, float* out, void* stream);
int twv_eval_elementwise64(int fn /*0 exp,1 log,2 exp for x <= 0 (the sampler's straight-line form)*/, const double* x, int64_t n, double* out, void* stream);

/* ======================================= Tacotron text -> mel inference =======================================
 * Replaces the graph synthesizer.py:56 builds with Tacotron.initialize(inputs, input_lengths, num_speakers, speaker_id,
 * rnn_decoder_test_mode=True) (tacotron/tacotron.py:36-235) and runs in one sess.run (synthesizer.py:160); default
 * hparams path: model_type 'deepvoice' with num_speakers > 1, attention_type 'bah_mon_norm'; also model_type 'simple', a single speaker,
 * and the attention types bah_mon, bah_norm, bah, luong, luong_scaled, loc_sen (not gmm, bah_mon_norm_hccho).  Fields = hparams.py:126-165. */
typedef struct {
    int32_t n_symbols, embedding_size, num_speakers, speaker_embedding_size;
    int32_t enc_prenet_sizes[2], enc_bank_size, enc_bank_channel_size, enc_proj_sizes[2], enc_proj_width, enc_highway_depth, enc_rnn_size;
    int32_t attention_size, attention_state_size;
    int32_t dec_prenet_sizes[2], dec_layer_num, dec_rnn_size;
    int32_t post_bank_size, post_bank_channel_size, post_proj_sizes[2], post_proj_width, post_highway_depth, post_rnn_size;
    int32_t num_mels, reduction_factor, num_freq, max_iters;
    int32_t model_simple;   /* 0: hparams.model_type 'deepvoice' (hparams.py:123, the default); 1: 'simple' (tacotron.py:85-90: the speaker embedding is
                             * concatenated inside the decoder, rnn_wrappers.py:425-432 / 455-463); read only when num_speakers > 1 */
    int32_t attention_type; /* hparams.attention_type (tacotron.py:127-144), TWV_ATT_*: 0 = 'bah_mon_norm' (hparams.py:145, the default).  The
                             * others run on the split decoder kernel only (decoder_groups 0, 1, 2, 4, 8, 16); 'luong' / 'luong_scaled'
                             * need attention_state_size == attention_size.  Appended last: callers of the older layout that zero the
                             * struct get the default.  A pass with caller-supplied alignments (twv_tacotron_infer_manual) runs none of the
                             * mechanisms: every type is served there at decoder_groups -1, 0, 1, 2, 4, 8 and 16. */
} twv_tacotron_dims;
enum { TWV_ATT_BAH_MON_NORM = 0, TWV_ATT_BAH_MON = 1, TWV_ATT_BAH_NORM = 2, TWV_ATT_BAH = 3, TWV_ATT_LUONG = 4, TWV_ATT_LUONG_SCALED = 5,
       TWV_ATT_LOC_SEN = 6 };
typedef struct twv_tacotron twv_tacotron;

int twv_tacotron_create(const twv_tacotron_dims* dims, twv_tacotron** out);          /* Tacotron(hparams) */
void twv_tacotron_destroy(twv_tacotron* h);
size_t twv_tacotron_blob_floats(const twv_tacotron* h);     /* canonical blob: checkpoint tensors in the order of weights.tacotron_specs,
                                                               batch-norm (gamma,beta,mean,var) replaced by the derived (inv, shift) pair */
size_t twv_tacotron_packed_bytes(const twv_tacotron* h);
size_t twv_tacotron_workspace_bytes(const twv_tacotron* h, int batch, int t_in);
int twv_tacotron_pack(const twv_tacotron* h, const float* blob, void* packed, void* stream);     /* saver.restore, synthesizer.py:69-70 */
/* one synthesize() pass (synthesizer.py:126-160): tokens (B,T_in) int32 (0 pad, 1 EOS), input_lengths (B), speaker ids (B) ->
 * mel (B, max_iters*r, num_mels), linear (B, max_iters*r, num_freq) or NULL, alignments (B, T_in, max_iters) or NULL. */
int twv_tacotron_infer(const twv_tacotron* h, const void* packed, const int32_t* tokens, const int32_t* lengths,
                       const int32_t* speaker_ids, int batch, int t_in, void* workspace, float* mel, float* linear,
                       float* alignments, int32_t* status, void* stream);

/* A pass with mel targets: Tacotron.initialize(..., mel_targets, ...) (tacotron/tacotron.py:36-37), whose decoder runs under
 * TacoTrainingHelper (tacotron/helpers.py:44-87) for exactly steps = t_out / r steps instead of max_iters.
 *   teacher_forced = 0  the reference's test_model (train_tacotron.py:154-155, rnn_decoder_test_mode=True): free-running, every step is fed
 *                       the last frame of its own output.  mel_targets gives nothing but the length and may be NULL.
 *   teacher_forced = 1  step 0 is fed the zero go-frame, step t = 1 .. steps - 1 the ground-truth frame mel_targets[n][t*r - 1][:]
 *                       (helpers.py:55, :86); no other target row is read (row t_out - 1 would feed a step after the last).  The output mels are the "ground-truth aligned" mels a vocoder is fine-tuned on.
 * mel_targets: device float[batch][t_out][num_mels].  t_out must be a multiple of reduction_factor and 1 <= t_out / r <= max_iters
 * (dynamic_decode stops at max_iters and the workspace is sized by it: the workspace of twv_tacotron_workspace_bytes serves any t_out).
 * Outputs: mel (B, t_out, num_mels), linear (B, t_out, num_freq) or NULL, alignments (B, t_in, t_out / r) or NULL.
 * The code is twv_tacotron_infer's -- which is this pass with t_out = max_iters * r and no targets -- so every decoder kernel, attention type,
 * model_type and option that serves infer serves this call, and the free-running pass of max_iters steps gives infer's bits.
 * Every layer stays in inference mode in BOTH modes: no dropout, moving-average batch normalisation.  The reference reaches teacher forcing only
 * together with its training-mode layers (is_training = not rnn_decoder_test_mode: prenet dropout, batch statistics); those belong to a
 * training step and are not built, so the teacher-forced pass is the evaluation-mode graph fed the targets, not the reference's training graph.
 * Padding frames are not masked (helpers.py:57-59).  Refused with TWV_E_INVALID before anything is launched: a null handle or buffer,
 * t_out % r != 0, t_out / r outside 1 .. max_iters, teacher_forced without mel_targets. */
int twv_tacotron_forward_targets(const twv_tacotron* h, const void* packed, const int32_t* tokens, const int32_t* lengths,
                                 const int32_t* speaker_ids, int batch, int t_in, const float* mel_targets, int t_out,
                                 int teacher_forced, void* workspace, float* mel, float* linear, float* alignments,
                                 int32_t* status, void* stream);
/* A pass with caller-supplied alignments: the inference graph's is_manual_attention / manual_alignments feeds (tacotron/tacotron.py:122-123),
 * under which AttentionWrapper's _compute_attention replaces the mechanism's alignments by manual_alignments[:, time, :] at every decoder
 * step (tacotron/rnn_wrappers.py:369-374); synthesizer.py:136-148 feeds saved alignments this way, :165-195 edited ones.
 * manual_alignments: device float[batch][steps][t_in] (the reference's [N, D, E]), 1 <= steps <= max_iters.  At step `it` the alignments used
 * for the context and carried as previous_alignments are manual_alignments[n][it][0 .. t_in) exactly as given: no mask past input_lengths,
 * no normalisation, no clipping.  The decoder runs free (the zero go-frame, then its own last frame) for exactly `steps` steps; everything
 * else is twv_tacotron_infer's pass, the post net and the linear projection on steps * r frames.  Outputs: mel (B, steps * r, num_mels),
 * linear (B, steps * r, num_freq) or NULL, alignments (B, t_in, steps) or NULL = the manual values transposed, bit for bit.  The mechanism is
 * not run and none of its tensors is read, whatever the attention_type (loc_sen's cumulative state included), so feeding a pass its own
 * alignments gives that pass's bits.  The values must be finite; that is not checked.
 * Kernels: tc_decoder_g_kernel (split) at decoder_groups 0, 1, 2, 4, 8, 16 with either decoder_local and decoder_split_all, tc_decoder_kernel
 * at -1, for every attention type and model_type.  The XCD-local kernel takes no manual alignments: decoder_groups = 0 goes the split route
 * here even where twv_tacotron_infer takes the resident kernel, and decoder_groups = 32 is TWV_E_UNSUPPORTED.  The workspace is
 * twv_tacotron_workspace_bytes', the same buffer serves both kinds of pass.
 * Refused before the device is looked at -- TWV_E_INVALID: a null handle, a null buffer other than linear / alignments, steps outside
 * 1 .. max_iters, batch < 1, t_in outside 1 .. 1024, no speaker_ids on a multi-speaker model; TWV_E_UNSUPPORTED: decoder_groups = 32.
 * TWV_E_UNSUPPORTED with the device's size known: the split kernel's geometry limits (LDS above 160 KiB, more than 512 workgroups).
 * twv_tacotron_manual_kernel_name: the kernel such a call launches, static strings as twv_tacotron_decoder_kernel_name's ("" where refused). */
int twv_tacotron_infer_manual(const twv_tacotron* h, const void* packed, const int32_t* tokens, const int32_t* lengths,
                              const int32_t* speaker_ids, int batch, int t_in, const float* manual_alignments, int steps,
                              void* workspace, float* mel, float* linear, float* alignments, int32_t* status, void* stream);
const char* twv_tacotron_manual_kernel_name(const twv_tacotron* h, int batch, int t_in);
/* The alignment edits of synthesizer.py:165-190 on the device, one launch: alignments (batch, t_in, steps) as a pass emits them ->
 * manual_out (batch, steps, t_in) as twv_tacotron_infer_manual reads them.  With d* = the first argmax over the steps of
 * alignments[n][e][:] for EVERY encoder row e, padded rows included (an all-zero row gives d* = 0):
 *   mode 0  the transpose (what saved alignments, --base_alignment_path, need)
 *   mode 1  synthesizer.py:167-173: zeros, then manual_out[n][d*][e] = 1
 *   mode 2  :175-183: the transpose squared elementwise (no renormalisation)
 *   mode 3  :185-190: the transpose, then manual_out[n][d*][e] = 1
 * Every output element is written.  TWV_E_INVALID: a null pointer, a size < 1, batch above 65535, another mode. */
int twv_tacotron_alignment_edit(const float* alignments, int batch, int t_in, int steps, int mode, float* manual_out, void* stream);

/* Tacotron.add_loss (tacotron.py:258-282) on device buffers: out = device double[4] = loss, mel_loss, linear_loss, loss_without_coeff.
 * mel / mel_targets (B, t_out, num_mels), linear / linear_targets (B, t_out, num_freq), loss_coeff (B) float (required: pass ones where the
 * examples carry none, datafeeder_tacotron.py:263).  prioritize_loss != 0: the band [int(165 / (sample_rate * 0.5) * num_freq),
 * int(5000 / (sample_rate * 0.5) * num_freq)) of the bins enters once more, linear_loss = 0.5 * (mean(l1) + mean(l1_priority)).
 * Every term is formed in float64 from the float32 inputs and summed in a tree whose order depends on the sizes only (no atomics): two calls
 * give the same bits.  Each input is read once; the block partials live in stream-ordered scratch (hipMallocAsync) for the call's duration. */
int twv_tacotron_loss(const float* mel, const float* linear, const float* mel_targets, const float* linear_targets,
                      const float* loss_coeff, int batch, int t_out, int num_mels, int num_freq, int prioritize_loss,
                      double sample_rate, double* out, void* stream);

/* ---- Tacotron batch staging: a batch's ragged arrays, packed, -> the padded arrays of a training step ----
 * `packed` (device, 16-byte aligned) is packed_words 32-bit words with four sections, each given by its first word: the tokens of every
 * utterance one after the other (int32, total_tokens), their mel rows (total_frames, num_mels) and linear rows (total_frames, num_freq) as
 * float32, and a table of `batch` twv_tacotron_feed_row at an even word.  table_host is the same table in host memory: every check is made on
 * it before anything is launched.  TWV_E_INVALID: a null argument, a size < 1 or above 2^20, an output above 2^38 words, a section or a
 * row's tokens / frames outside the buffer, a row with more tokens than t_in or more frames than t_out, a misaligned `packed`, table or
 * target.  Out, every element written (the padding is stored): inputs (batch, t_in) int32 and mel_targets (batch, t_out, num_mels) /
 * linear_targets (batch, t_out, num_freq), padded with 0; input_lengths, loss_coeff, speaker_id (batch) -- what datafeeder_tacotron.py:
 * 269-309 `_prepare_batch` builds on the host, bit for bit.  The targets must be 16-byte aligned.  No atomics. */
typedef struct twv_tacotron_feed_row {
    int64_t token_offset, frame_offset;   /* in tokens / frames from the start of the section */
    int32_t n_tokens, n_frames, speaker_id;
    float loss_coeff;
} twv_tacotron_feed_row;
int twv_tacotron_batch_stage(const void* packed, const twv_tacotron_feed_row* table_host, long long packed_words, long long tokens_at,
                             long long mel_at, long long linear_at, long long table_at, long long total_tokens, long long total_frames,
                             int batch, int t_in, int t_out, int num_mels, int num_freq, int32_t* inputs, int32_t* input_lengths,
                             float* mel_targets, float* linear_targets, float* loss_coeff, int32_t* speaker_id, void* stream);

/* ---- WaveNet crop staging: a batch's random crops cut from a corpus that lives on the device ----
 * audio_pool (device, audio_floats float32) holds every example's samples, mel_pool (device, mel_floats float32) every example's mel rows
 * (n_frames, num_mels) packed densely; row i of the table says where example i starts in each pool (offsets in floats), how many frames it
 * has (its audio is n_frames * hop_size samples) and its speaker id.  picks is (batch, 2) int32: the example and the crop's first frame.
 * The table and the picks are given twice, in host and in device memory: every check is made on the host copies before anything is
 * launched, the kernel reads the device copies.  TWV_E_INVALID: a null argument, a size < 1 or above 2^20, an output above 2^38 words, an
 * example outside [0, n_examples), start < 0 or start + frames > n_frames, a picked row whose audio or mel range leaves its pool, audio or
 * local_condition not 16-byte aligned.  Out, every element written by ONE launch: audio (batch, frames * hop_size) =
 * audio_pool[audio_offset + start * hop_size ...], local_condition (batch, frames, num_mels) = rows start .. start + frames of the
 * example's mels, gc_ids (batch) = the rows' speaker ids -- what datafeeder_wavenet.py:150-156 cuts on the host, bit for bit.  Nothing
 * outside the two ranges a picked row names is read.  No atomics. */
typedef struct twv_wavenet_feed_row {
    int64_t audio_offset, mel_offset;     /* in floats from the start of the pool */
    int32_t n_frames, speaker_id;
} twv_wavenet_feed_row;
int twv_wavenet_crop_stage(const float* audio_pool, long long audio_floats, const float* mel_pool, long long mel_floats,
                           const twv_wavenet_feed_row* table_host, const twv_wavenet_feed_row* table_dev, int n_examples,
                           const int32_t* picks_host, const int32_t* picks_dev, int batch, int frames, int hop_size, int num_mels,
                           float* audio, float* local_condition, int32_t* gc_ids, void* stream);

/* ---- Tacotron decoder gradients: the vector-Jacobian product of the teacher-forced decoder ----
 * Host only: where a twv_tacotron_infer / twv_tacotron_forward_targets call of (batch, t_in) left the pieces the decoder reads from the
 * encoder side, as (offset, count) in floats from the start of its workspace.  which = "memory" (batch, t_in, 2 * enc_rnn_size; zero past
 * each length), "keys" (batch, t_in, attention_size) or "decoder_init" (batch, attention_state_size + dec_layer_num * dec_rnn_size: the
 * attention cell's state, then each residual GRU's).  Any other name, a null argument or a (batch, t_in) the passes refuse: TWV_E_INVALID. */
int twv_tacotron_workspace_view(const twv_tacotron* h, int batch, int t_in, const char* which, long long* offset_floats, long long* floats);

/* A gradient handle for (batch, t_in, steps) on the model of `h` (which is not kept).  Host only; every refusal comes before the device is
 * touched.  TWV_E_INVALID: null arguments, steps outside 1 .. max_iters, batch < 1, t_in outside 1 .. 1024.  TWV_E_UNSUPPORTED: what is not
 * built -- attention types other than bah_mon_norm and bah_mon, model_type 'simple', dec_prenet_sizes or num_mels above 512.
 * twv_tacotron_decoder_grad_route: a label of the kernels and sizes in use ("kernel=tg_bptt attention=... workgroups_per_utterance=1 ..."). */
typedef struct twv_tacotron_decoder_grad twv_tacotron_decoder_grad;
int twv_tacotron_decoder_grad_create(const twv_tacotron* h, int batch, int t_in, int steps, twv_tacotron_decoder_grad** out);
/* The same with every attention type twv_tacotron_create accepts (bah_norm, bah, luong, luong_scaled, loc_sen beside the two monotonic
 * types); model_type 'simple' and the size limits are refused as above.  Host only.  For the monotonic types the handle is the one
 * twv_tacotron_decoder_grad_create makes (same workspace, label, kernels).  Every other twv_tacotron_decoder_grad_* call takes either kind
 * of handle; twv_tacotron_decoder_grad_reshape validates as the call that made the handle did. */
int twv_tacotron_decoder_grad_create_any(const twv_tacotron* h, int batch, int t_in, int steps, twv_tacotron_decoder_grad** out);
void twv_tacotron_decoder_grad_destroy(twv_tacotron_decoder_grad* g);
size_t twv_tacotron_decoder_grad_workspace_bytes(const twv_tacotron_decoder_grad* g);
const char* twv_tacotron_decoder_grad_route(const twv_tacotron_decoder_grad* g);
/* The handle at other sizes: accepts exactly what twv_tacotron_decoder_grad_create accepts for the handle's model and refuses the rest with
 * the same codes and words (the LDS bound on t_in included).  Host only.  Kept: the rocBLAS handle, the events, the timing flag.  Follows the
 * sizes: twv_tacotron_decoder_grad_workspace_bytes, the label's LDS sizes.  The backward is refused until a forward at the new sizes, as
 * after _create.  A refused call leaves the handle unchanged.  A reshaped handle's runs give the bits of a newly created handle's,
 * whatever the handle ran before and whatever the workspace holds. */
int twv_tacotron_decoder_grad_reshape(twv_tacotron_decoder_grad* g, int batch, int t_in, int steps);
/* The teacher-forced decoder forward (recorded) and its backward through time.
 * In:  blob          the canonical weights on the device (twv_tacotron_blob_floats floats, the order of tacotron_specs)
 *      memory        (batch, t_in, 2 * enc_rnn_size), decoder_init (batch, AS + layers * DR), lengths (batch) int32
 *      mel_targets   (batch, steps * r, num_mels): step 0 is fed zeros, step t the row t * r - 1 (helpers.py:80-87)
 *      d_mel         (batch, steps * r, num_mels): the cotangent on the mel output
 *      mask1, mask2  NULL, or (batch, steps, dec_prenet_sizes[i]) multipliers applied after each decoder-prenet relu (TF dropout: 0 or
 *                    1 / keep_prob; the caller draws them).  NULL masks give the evaluation graph.
 * Scratch: workspace (twv_tacotron_decoder_grad_workspace_bytes, in any state: no word is read before this call wrote it), status (4 x int32,
 *      zeroed), stream.
 * Out: mel_out       (batch, steps * r, num_mels): with NULL masks the teacher-forced twv_tacotron_forward_targets mel up to summation order
 *      grad_blob     the layout of blob: zeroed, then the gradient of every decoder-side tensor (memory_layer/kernel .. decoder/
 *                    output_projection_wrapper/bias) written at the tensor's place; every other tensor reads 0
 *      d_memory      (batch, t_in, 2 * enc_rnn_size), exactly 0 past each length; d_init (batch, AS + layers * DR)
 * One workgroup per utterance runs the recurrence and no workgroup waits for another; no atomics: two runs give the same bits, and an
 * utterance's d_memory / d_init rows are the same bits alone and inside a batch. */
int twv_tacotron_decoder_grad_run(twv_tacotron_decoder_grad* g, const float* blob, const float* memory, const float* decoder_init,
                                  const int32_t* lengths, const float* mel_targets, const float* d_mel, const float* mask1,
                                  const float* mask2, void* workspace, int32_t* status, void* stream, float* mel_out,
                                  float* grad_blob, float* d_memory, float* d_init);
/* The two halves of twv_tacotron_decoder_grad_run as calls of their own (a training step runs every forward before any backward): the
 * arguments are the run's.  The tape stays in `workspace` between the two, so the backward is given the forward's workspace, blob, memory,
 * decoder_init and lengths.  _run is _forward followed by _backward.  _backward on a handle with no forward since create: TWV_E_INVALID. */
int twv_tacotron_decoder_grad_forward(twv_tacotron_decoder_grad* g, const float* blob, const float* memory, const float* decoder_init,
                                      const int32_t* lengths, const float* mel_targets, const float* mask1, const float* mask2,
                                      void* workspace, int32_t* status, void* stream, float* mel_out);
int twv_tacotron_decoder_grad_backward(twv_tacotron_decoder_grad* g, const float* blob, const float* memory, const float* decoder_init,
                                       const int32_t* lengths, const float* d_mel, void* workspace, int32_t* status, void* stream,
                                       float* grad_blob, float* d_memory, float* d_init);
/* measurement: with timing on, a run records events at its phase boundaries; twv_tacotron_decoder_grad_phase_ms waits for the last run and
 * gives ms3 = milliseconds of the recording forward, the backward through time, the weight-gradient products (TWV_E_INVALID before such a run) */
int twv_tacotron_decoder_grad_set_timing(twv_tacotron_decoder_grad* g, int on);
int twv_tacotron_decoder_grad_phase_ms(twv_tacotron_decoder_grad* g, double* ms3);
/* the derivative of add_loss's mel term (tacotron.py:258-282) with respect to mel: d_mel = sign(mel - mel_targets) * loss_coeff[n] /
 * (batch * t_out * num_mels), 0 where the difference is 0.  All of (batch, t_out, num_mels) but loss_coeff (batch). */
int twv_tacotron_mel_loss_grad(const float* mel, const float* mel_targets, const float* loss_coeff, int batch, int t_out, int num_mels,
                               float* d_mel, void* stream);

/* ---- Tacotron encoder and post-net gradients: the vector-Jacobian product of one CBHG, instantiated twice ----
 * twv_tacotron_workspace_view also answers "before_highway" (batch, enc_prenet_sizes[1]) and "encoder_rnn_init" (batch, 2 * enc_rnn_size =
 * [fw | bw]): the speaker-dependent pieces a multi-speaker 'deepvoice' pass leaves in its workspace (TWV_E_INVALID for a model without them).
 *
 * A handle for (model, which, batch, t): t = t_in for TWV_CBHG_ENCODER, T_out for TWV_CBHG_POST.  Host only; every refusal comes before the
 * device is touched.  TWV_E_INVALID: null arguments, another `which`, batch < 1, t_in outside 1 .. 1024, T_out outside 1 .. max_iters * r.
 * TWV_E_UNSUPPORTED: model_type 'simple', proj_width above 16 (the row kernel stages 8 + width - 1 rows).  The attention type is not looked at.
 * twv_tacotron_cbhg_grad_route: a label ("kernel=cg_bigru side=encoder|post workgroups_per_utterance=2 threads=512 weights=registers ..."). */
#define TWV_CBHG_ENCODER 0
#define TWV_CBHG_POST 1
typedef struct twv_tacotron_cbhg_grad twv_tacotron_cbhg_grad;
int twv_tacotron_cbhg_grad_create(const twv_tacotron* h, int which, int batch, int t, twv_tacotron_cbhg_grad** out);
void twv_tacotron_cbhg_grad_destroy(twv_tacotron_cbhg_grad* g);
size_t twv_tacotron_cbhg_grad_workspace_bytes(const twv_tacotron_cbhg_grad* g);
const char* twv_tacotron_cbhg_grad_route(const twv_tacotron_cbhg_grad* g);
/* The handle at another (batch, t), as twv_tacotron_decoder_grad_reshape: what twv_tacotron_cbhg_grad_create accepts for the handle's model
 * and side, the same refusals; the batch-norm mode, its variables pointer and the handle's device buffers (their sizes are sums of channel
 * counts) are kept with the rocBLAS handle, the events and the timing flag. */
int twv_tacotron_cbhg_grad_reshape(twv_tacotron_cbhg_grad* g, int batch, int t);
/* The encoder (embedding, prenet, encoder CBHG), recorded, and its backward.
 * In:  blob            the canonical weights on the device; tokens (batch, t_in) int32, lengths (batch) int32
 *      before_highway  (batch, enc_prenet_sizes[1]) and rnn_init (batch, 2 * enc_rnn_size), or NULL each (a single-speaker model)
 *      mask1, mask2    NULL, or (batch, t_in, enc_prenet_sizes[i]) multipliers after each prenet relu (dropout); NULL = the evaluation graph
 *      d_memory        (batch, t_in, 2 * enc_rnn_size): the cotangent on the encoder output; rows past a length are not read
 * Scratch: workspace (twv_tacotron_cbhg_grad_workspace_bytes, in any state), status (4 x int32, zeroed), stream.
 * Out: memory_out      the recorded encoder output, exactly 0 past each length
 *      grad_blob       the layout of blob: zeroed, then the gradients of embedding (row 0 exactly 0: the forward reads the <PAD> row as
 *                      zeros), prenet/ * and encoder_cbhg/ *; a batch_normalization slot holds (d_inv, d_shift) of the derived pair
 *      d_before_highway, d_rnn_init   as their inputs (required where the input is given, not touched otherwise)
 * Padded rows pass through the prenet and the convolutions like any other row (the reference does not mask them); only the GRUs are
 * masked.  No atomics, no workgroup waits for another: two runs give the same bits, and an utterance's outputs are the same bits alone
 * and inside a batch. */
int twv_tacotron_encoder_grad_run(twv_tacotron_cbhg_grad* g, const float* blob, const int32_t* tokens, const int32_t* lengths,
                                  const float* before_highway, const float* rnn_init, const float* mask1, const float* mask2,
                                  const float* d_memory, void* workspace, int32_t* status, void* stream, float* memory_out,
                                  float* grad_blob, float* d_before_highway, float* d_rnn_init);
/* The post net (post CBHG, linear-spectrogram layer), recorded, and its backward.  mel (batch, t_out, num_mels), d_linear and linear_out
 * (batch, t_out, num_freq); grad_blob as above with post_cbhg/ * and the linear layer; d_mel (batch, t_out, num_mels) the cotangent on mel. */
int twv_tacotron_postnet_grad_run(twv_tacotron_cbhg_grad* g, const float* blob, const float* mel, const float* d_linear, void* workspace,
                                  int32_t* status, void* stream, float* linear_out, float* grad_blob, float* d_mel);
/* The halves of the two runs as calls of their own, as for the decoder: the run's arguments; the backward is given the forward's workspace,
 * blob and inputs (tokens and lengths; mel), and d_before_highway / d_rnn_init where the forward was given their inputs.  A backward on a
 * handle with no forward since create or set_mode, or on a handle of the other kind: TWV_E_INVALID. */
int twv_tacotron_encoder_grad_forward(twv_tacotron_cbhg_grad* g, const float* blob, const int32_t* tokens, const int32_t* lengths,
                                      const float* before_highway, const float* rnn_init, const float* mask1, const float* mask2,
                                      void* workspace, int32_t* status, void* stream, float* memory_out);
int twv_tacotron_encoder_grad_backward(twv_tacotron_cbhg_grad* g, const float* blob, const int32_t* tokens, const int32_t* lengths,
                                       const float* d_memory, void* workspace, int32_t* status, void* stream, float* grad_blob,
                                       float* d_before_highway, float* d_rnn_init);
int twv_tacotron_postnet_grad_forward(twv_tacotron_cbhg_grad* g, const float* blob, const float* mel, void* workspace, int32_t* status,
                                      void* stream, float* linear_out);
int twv_tacotron_postnet_grad_backward(twv_tacotron_cbhg_grad* g, const float* blob, const float* mel, const float* d_linear, void* workspace,
                                       int32_t* status, void* stream, float* grad_blob, float* d_mel);
/* The batch norm of a handle's passes.  TWV_BN_INFERENCE, the default: y = a * inv + shift with the blob's pair (the moving
 * statistics).  TWV_BN_BATCH: tf.layers.batch_normalization(training=True) -- each of the bank + 2 batch norms takes the mean and the biased
 * variance of its input over ALL batch * t rows (padded rows too; float64 sums in a fixed order, each statistic rounded once to float32),
 * derives its pair from them and from gamma and beta in twv_tacotron_refold's rounding sequence, and the backward goes through the
 * statistics.  `variables` is the training vector on the device (twv_tacotron_train_floats; gamma and beta are read from it at every
 * forward, so it must outlive the mode); it is not looked at in inference mode.  In batch mode a batch_normalization slot of grad_blob holds
 * (d_gamma, d_beta) themselves (twv_tacotron_grad_convert_batch), and an utterance's outputs depend on the whole batch.
 * twv_tacotron_cbhg_grad_batch_stats copies the statistics of the last batch-mode forward to `out` on the device:
 * twv_tacotron_cbhg_grad_batch_stats_floats floats, per batch norm in the order bank 1 .. K, proj_1, proj_2 a (2, C) piece = (mean, variance).
 * TWV_E_INVALID: another mode, batch mode without variables, statistics before a batch-mode forward. */
#define TWV_BN_INFERENCE 0
#define TWV_BN_BATCH 1
int twv_tacotron_cbhg_grad_set_mode(twv_tacotron_cbhg_grad* g, int mode, const float* variables);
size_t twv_tacotron_cbhg_grad_batch_stats_floats(const twv_tacotron_cbhg_grad* g);
int twv_tacotron_cbhg_grad_batch_stats(const twv_tacotron_cbhg_grad* g, float* out, void* stream);
/* measurement, as for the decoder: ms4 = the recording forward, the GRUs' backward through time, the row-wise backward (pointwise kernels
 * and dx products), the weight-gradient products */
int twv_tacotron_cbhg_grad_set_timing(twv_tacotron_cbhg_grad* g, int on);
int twv_tacotron_cbhg_grad_phase_ms(twv_tacotron_cbhg_grad* g, double* ms4);
/* the derivative of add_loss's linear term (tacotron.py:258-282) with respect to linear_outputs: s = sign(linear - target) * loss_coeff[n]
 * (0 where the difference is 0); d_linear = s / (N T F), or with prioritize_loss s * (0.5 / (N T F) + [lo <= f < hi] * 0.5 / (N T (hi - lo)))
 * with the band of twv_tacotron_loss. */
int twv_tacotron_linear_loss_grad(const float* linear, const float* linear_targets, const float* loss_coeff, int batch, int t_out,
                                  int num_freq, int prioritize_loss, double sample_rate, float* d_linear, void* stream);

/* ---- Tacotron training step: the speaker side's gradient and the training vector ----
 * The gradient of the speaker tensors from the three cotangents the other passes hand back: d_before_highway (batch, enc_prenet_sizes[1])
 * and d_encoder_rnn_init (batch, 2 * enc_rnn_size) of twv_tacotron_encoder_grad_run, d_init (batch, attention_state_size + dec_layer_num *
 * dec_rnn_size) of twv_tacotron_decoder_grad_run.
 * 'deepvoice' with a speaker embedding: per dense layer i (0 <- d_before_highway, 1 <- d_encoder_rnn_init, 2 .. <- the column blocks of
 * d_init) z_i = e W_i + b_i is recomputed from blob and the rows e = speaker_embedding[speaker_ids]; dz_i = dy_i / (1 + |z_i|)^2 (softsign),
 * dW_i = e^T dz_i, db_i = the column sum of dz_i, d_e = sum_i dz_i W_i^T, d speaker_embedding[s] = the sum of d_e[n] over speaker_ids[n] = s.
 * speaker_embedding_size 1: the five get_embed tables, d table_i[s] = the sum of the cotangent's rows of speaker s.
 * Only the speaker tensors' ranges of grad_blob (the layout of blob) are written.  scratch: twv_tacotron_speaker_grad_scratch_bytes of the
 * caller's, in any state.  No atomics; every sum over utterances runs in utterance order, in float64, rounded once: equal inputs give equal
 * bits, and a speaker no utterance names gets a row of exact zeros (an id outside 0 .. num_speakers - 1 names nobody).
 * Host-side refusals, before the device is touched: null arguments or batch < 1 TWV_E_INVALID; a single-speaker model TWV_E_INVALID (it
 * has no speaker tensors); model_type 'simple' TWV_E_UNSUPPORTED. */
size_t twv_tacotron_speaker_grad_scratch_bytes(const twv_tacotron* h, int batch);
int twv_tacotron_speaker_grad(const twv_tacotron* h, const float* blob, const int32_t* speaker_ids, int batch,
                              const float* d_before_highway, const float* d_encoder_rnn_init, const float* d_init, void* scratch,
                              float* grad_blob, void* stream);
/* The training vector: every tensor of tacotron_specs in canonical order, a batch_normalization entry as its (4, C) checkpoint tensor
 * (gamma, beta, moving_mean, moving_variance) where the blob holds the derived (inv, shift) pair: twv_tacotron_train_floats =
 * twv_tacotron_blob_floats + 2 C per batch norm.
 * twv_tacotron_refold: variables -> blob, the bits of tacotron.flatten (inv = (1 / sqrt(var + 1e-3)) * gamma, shift = beta - mean * inv, every
 * operation rounded to float32 in that order); re-pack (twv_tacotron_pack) before the next pass.
 * twv_tacotron_grad_convert: a blob-shaped gradient -> the gradient of the training vector: (d_inv, d_shift) -> d_gamma = rsqrt(var + 1e-3)
 * (d_inv - mean d_shift), d_beta = d_shift (float64 inside), exact zeros for the moving statistics, every other range copied.
 * Null arguments: TWV_E_INVALID. */
size_t twv_tacotron_train_floats(const twv_tacotron* h);
int twv_tacotron_refold(const twv_tacotron* h, const float* variables, float* blob, void* stream);
int twv_tacotron_grad_convert(const twv_tacotron* h, const float* variables, const float* grad_blob, float* grad_variables, void* stream);
/* The training-mode step's own pieces.
 * twv_tacotron_grad_convert_batch: twv_tacotron_grad_convert for a gradient whose batch_normalization slots hold (d_gamma, d_beta) already
 * (passes in TWV_BN_BATCH mode): they are copied, the moving statistics get exact zeros.
 * twv_tacotron_moving_update: tf's assign_moving_average without zero-debias on the moving mean and variance of every batch norm of both
 * CBHGs in the training vector: m <- m - (m - batch) * (float)(1 - momentum), each operation rounded to float32 (the reference's momentum is
 * 0.99); encoder_stats / post_stats are twv_tacotron_cbhg_grad_batch_stats of the two handles.
 * twv_dropout_mask: n dropout multipliers from a counter-based generator -- element i depends on (seed, step, site, i) alone:
 * key = mix(seed + G (4 step + site)), z = mix(key + G (i + 1)), u = (z >> 40) 2^-24, with mix the splitmix64 finaliser and G =
 * 0x9E3779B97F4A7C15; out[i] = (float)(1 / (1 - rate)) where u >= (float)rate, else 0.  site 0 .. 3 = encoder prenet 1, 2, decoder prenet 1, 2.
 * TWV_E_INVALID: null arguments, momentum outside [0, 1], n < 1, step < 0, another site, rate outside [0, 1). */
int twv_tacotron_grad_convert_batch(const twv_tacotron* h, const float* grad_blob, float* grad_variables, void* stream);
int twv_tacotron_moving_update(const twv_tacotron* h, float* variables, const float* encoder_stats, const float* post_stats, double momentum,
                               void* stream);
int twv_dropout_mask(float* out, int64_t n, uint64_t seed, int64_t step, int site, double rate, void* stream);

/* launch geometry (performance only, results are bit-identical): "decoder_groups" = 0 auto (the XCD-resident decoder kernel wherever it
 * fits -- batch <= 32, t_in <= 512, 256 CUs, decoder widths divisible by 4, not model_type 'simple', attention_type bah_mon_norm -- else the split kernel with 16 / 8 / 4
 * workgroups per utterance), 1/2/4/8/16 = the split kernel with that many workgroups per utterance, 32 = the XCD-resident kernel or an
 * error, -1 = the single-workgroup kernel.  "gemm_group" / "highway_stack" / "gemm_valu": 0 / 0 / 1 select the older launch forms of the
 * dense layers (one launch per problem, one per highway layer, the VALU kernel) for A/B runs and cross-checks. */
int twv_tacotron_set_option(twv_tacotron* h, const char* name, int value);
/* optional decoder phase timestamps (tuning aid): device uint64[max_iters][16], s_memtime ticks of utterance 0's workgroup at the
 * phase boundaries of every decoder step (prenet, attention GRU, query, score, recurrence, context, projection, residual GRUs,
 * output).  NULL disables. */
int twv_tacotron_set_profile_buffer(twv_tacotron* h, void* dev_u64);
/* measurement aid for bench.py's `tacotron.roofline` (no reference counterpart): after twv_tacotron_set_option(h, "gemm_timing", 1)
 * every dense contraction of the pass (CBHG conv banks / projections / highways of tacotron/modules.py:25-74, the attention keys and the
 * linear projection) is bracketed by HIP events on its stream; this returns the useful FLOPs (2*rows*K*N), the summed kernel time
 * and the launch count since then. */
int twv_tacotron_gemm_stats(twv_tacotron* h, double* flop, double* ms, int64_t* launches);
/* the decoder kernel twv_tacotron_infer launches for this (handle, batch, t_in, options) on the current device:
 * "tc_decoder_x_kernel" (XCD-resident), "tc_decoder_g_kernel" (split) or "tc_decoder_kernel" (static string; measurement label, bench.py);
 * "" where infer refuses the options (an attention_type other than bah_mon_norm with decoder_groups -1 or 32) */
const char* twv_tacotron_decoder_kernel_name(const twv_tacotron* h, int batch, int t_in);

/* ======================================= WaveNet teacher-forced training step =======================================
 * Replaces one `sess.run([net.loss, net.optimize])` of train_vocoder.py:155-181 for the scalar-input (MoL) model:
 * add_loss (wavenet/model.py:247-312: drop last sample, create_upsample, 'valid' convolution network with the
 * front-sliced local condition, discretized_mix_logistic_loss(num_class=2**16) mean) and add_optimizer
 * (model.py:314-346: Adam with TF defaults, then ExponentialMovingAverage(0.9999).apply).  Parameters and gradients are
 * flat float32 device arrays in the canonical checkpoint order (twv_wavenet_blob_floats / weights.tensor_specs).
 * Data-parallel training all-reduces `grads` between the two calls (host side, RCCL). */
typedef struct twv_wavenet_trainer twv_wavenet_trainer;
/* batch = hparams.wavenet_batch_size, n_samples = crop length fed by DataFeederWavenet (a multiple of the hop size) */
int twv_wavenet_train_create(const twv_wavenet_dims* dims, int batch, int n_samples, twv_wavenet_trainer** out);
/* the same with the widest residual_channels = dilation_channels the caller is prepared to run: max_width 32, 64 or 128 (anything else
 * is TWV_E_INVALID).  With 32 it is twv_wavenet_train_create (which calls it) and refuses with that function's text; above 32 it accepts
 * equal widths of 32, 64 and 128 up to max_width and refuses the rest with "... 32, 64 or 128 only (got R, D)".  A width-32 handle is
 * the same handle from either function; every other twv_wavenet_train_* call takes a handle of any width.  At 64 and 128 the step keeps
 * three width-sized arrays per layer: twv_wavenet_train_workspace_bytes says how much (tens of GB at 30 layers, 64 x 7800, width 128). */
int twv_wavenet_train_create_w(const twv_wavenet_dims* dims, int batch, int n_samples, int max_width, twv_wavenet_trainer** out);
void twv_wavenet_train_destroy(twv_wavenet_trainer* h);
size_t twv_wavenet_train_param_floats(const twv_wavenet_trainer* h);
size_t twv_wavenet_train_workspace_bytes(const twv_wavenet_trainer* h);
/* forget which workspace has been cleared: the next twv_wavenet_train_loss_grad clears the one it is given.  Call it when a workspace
 * was freed and re-allocated (a caching allocator may hand out the same address) or written by anything else between two steps. */
int twv_wavenet_train_reset_workspace(twv_wavenet_trainer* h);
int twv_wavenet_train_output_width(const twv_wavenet_trainer* h);          /* n_samples - receptive_field (model.py:135) */
/* host-only: which kernel families twv_wavenet_train_loss_grad runs for this trainer, as a string the handle owns:
 *   "lc=<fused|staged> head=<skinny+c2bwd|skinny|gemm> loss=<mol<10>|mol<0>|softmax> nsplit=<n> width=<32|64|128> carve_floats=<n>"
 * lc: frame-rate lc projections inside the layer kernels, or the materialised upsampler; head: conv1d_2 as the skinny kernel (with or
 * without its fused backward) or library GEMMs; nsplit: K slabs of the wide weight gradients; carve_floats: the floats loss_grad takes
 * from the start of the workspace (workspace_bytes / 4 is at least that).  A label for tests and measurements. */
const char* twv_wavenet_train_route(const twv_wavenet_trainer* h);
/* loss (device float[1]) and d loss / d params (device float[param_floats], overwritten).
 * audio (B, n_samples) float in [-1,1]; lc (B, n_samples/hop, lc_channels); gc_ids (B) int32.
 * workspace: workspace_bytes of device memory that belongs to the trainer between calls (a pointer seen for the first time is
 * cleared once; parts of it -- activation rows in front of a layer's receptive offset -- are never written afterwards and read as zeros). */
int twv_wavenet_train_loss_grad(twv_wavenet_trainer* h, const float* params, const float* audio, const float* lc,
                                const int32_t* gc_ids, void* workspace, float* loss, float* grads, void* stream);
/* model.py:300-312 optional L2 term over the non-bias variables (after loss_grad): loss += strength*sum(w^2)/2, grads += strength*w.
 * workspace: the trainer's workspace (the call uses a scratch region of its own at the end of it: nothing loss_grad keeps there is touched). */
int twv_wavenet_train_l2(twv_wavenet_trainer* h, const float* params, double strength, void* workspace, float* loss, float* grads,
                         void* stream);
/* model.py:330-331 tf.clip_by_global_norm on the flat gradient buffer: grads <- grads*pre_scale * clip_norm / max(||grads*pre_scale||, clip_norm).
 * scratch: n + 1024 floats of the caller's -- NOT the training workspace (rows of that one must stay as loss_grad left them). */
int twv_clip_by_global_norm(float* grads, int64_t n, double pre_scale, double clip_norm, void* scratch, void* stream);
/* tf.train.AdamOptimizer.apply_gradients (t = 1-based update count) on grads*grad_scale, then the EMA shadow update. */
int twv_adam_ema_step(float* params, const float* grads, float* m, float* v, float* ema, int64_t n, double lr, double beta1,
                      double beta2, double eps, int64_t t, double ema_decay, double grad_scale, void* stream);

/* ======================================= WaveNet scoring: per-sample negative log-likelihood =======================================
 * The add_loss graph with reduce=False (wavenet/model.py:247-312: drop last sample, create_upsample, 'valid' convolutions with the
 * local condition sliced from the front of every layer, model.py:79-80; targets audio[rf:]; wavenet/mixture.py:27-81
 * discretized_mix_logistic_loss(reduce=False), or model.py:257-296 softmax cross-entropy for the one-hot model) on a batch of WINDOWS:
 * forward only, no gradient, no mean.  For a hop-aligned start s the graph on the crop audio[s : s+n], mel[s/hop : (s+n)/hop] gives the
 * whole utterance's values at positions s+rf .. s+n-1 (the front slice is shift-invariant at hop multiples), so the host scores an
 * utterance of any length as windows with a halo of ceil(rf / hop) * hop samples (score.py) and memory is bounded by (slots, window). */
typedef struct twv_wavenet_scorer twv_wavenet_scorer;
/* accepts what twv_wavenet_train_create accepts (80 mel channels, gc with a cardinality, out_channels = 3*nr <= 96 or
 * quantization_channels in [2, 512]) at residual_channels = dilation_channels = 32, and the same at 64 and 128 (the training step is
 * built for 32 only); unequal or other widths and everything else are TWV_E_UNSUPPORTED, as is slots * window_samples * 256 >= 2^31
 * where the local condition is projected at frame rate (three upsampling stages, 32 <= hop <= 512), at every width.  TWV_E_INVALID: window_samples not a multiple of
 * the hop size (datafeeder_wavenet.py:38) or <= the receptive field (model.py:31-39). */
int twv_wavenet_score_create(const twv_wavenet_dims* dims, int slots, int window_samples, twv_wavenet_scorer** out);
void twv_wavenet_score_destroy(twv_wavenet_scorer* h);
size_t twv_wavenet_score_workspace_bytes(const twv_wavenet_scorer* h);      /* a function of (dims, slots, window_samples) only */
int twv_wavenet_score_output_width(const twv_wavenet_scorer* h);            /* window_samples - receptive_field (model.py:135) */
/* host-only label for tests and measurements, a string the handle owns:
 *   "lc=<fused|staged> head=<skinny|gemm> loss=<mol<10>|mol<0>|softmax> width=<32|64|128> carve_floats=<n>" (lc as twv_wavenet_train_route) */
const char* twv_wavenet_score_route(const twv_wavenet_scorer* h);
/* host only: where a workspace holds two intermediate arrays after twv_wavenet_score_windows, for tests that look at more than the
 * loss.  name "zc": the stacked skip input ZC[(b, p)][l * dilation_channels + j] (model.py:94-96: layer l's z of the last
 * window_samples - rf rows), rows = slots * (window_samples - rf), cols = n_layers * dilation_channels; "y": the raw network output
 * (model.py:150-165), cols = out_channels or quantization_channels.  Row-major at offset_floats floats from the workspace's start;
 * rows p >= lengths[b] - rf of a slot are not written.  Any other name is TWV_E_INVALID. */
int twv_wavenet_score_view(const twv_wavenet_scorer* h, const char* name, long long* offset_floats, long long* rows, long long* cols);
/* nll (slots, window_samples - rf) float32, overwritten: nll[b][p] = the loss term of target audio[b][p + rf] (model.py:286-296) for
 * p < lengths_host[b] - rf, 0 for the positions slot b does not have.  params: the flat blob of twv_wavenet_train_param_floats floats
 * in the order of weights.tensor_specs (a trainer's params or EMA shadows as they are).  audio (slots, window_samples) float in [-1,1];
 * lc (slots, window_samples/hop, 80); gc_ids (slots) int32, a valid id for idle slots too.  lengths_host (HOST, slots): samples in each
 * slot from its start -- a multiple of the hop size in (rf, window_samples], or 0 for an idle slot; anything else is TWV_E_INVALID
 * before anything is launched.  Rows past a slot's length are neither read nor written.  workspace: workspace_bytes of device memory in
 * any state (nothing relies on its contents). */
int twv_wavenet_score_windows(twv_wavenet_scorer* h, const float* params, const float* audio, const float* lc, const int32_t* gc_ids,
                              const int32_t* lengths_host, void* workspace, float* nll, void* stream);
/* out_double2 (device double[2], overwritten) = (sum, count) of nll[b][keep_from_host[b] .. keep_to_host[b] - 1] over the slots
 * (0 <= from <= to <= width, else TWV_E_INVALID): model.py:290's mean is sum / count over the windows of a list.  Float64, one fixed
 * order of additions: two runs give the same bits. */
int twv_wavenet_score_reduce(const float* nll, const int32_t* keep_from_host, const int32_t* keep_to_host, int slots, int width,
                             double* out_double2, void* stream);

/* ======================================= spectrogram -> waveform (Griffin-Lim) =======================================
 * Replaces synthesizer.py:258 `inv_linear_spectrogram(wav.T, hparams)` (utils/audio.py:77-92, 127-146, 27-30): denormalise,
 * dB -> amplitude, ** power, Griffin-Lim with librosa's stft/istft conventions, inverse pre-emphasis.  FFTs by hipFFT. */
typedef struct twv_griffin_lim twv_griffin_lim;
/* n_fft = hparams.fft_size, hop = hop_size, win_length = win_size; n_frames spectrogram frames per utterance */
int twv_griffin_lim_create(int n_fft, int hop, int win_length, int n_frames, int batch, twv_griffin_lim** out);
void twv_griffin_lim_destroy(twv_griffin_lim* h);
int twv_griffin_lim_samples(const twv_griffin_lim* h);                 /* hop * (n_frames - 1) samples per utterance */
size_t twv_griffin_lim_workspace_bytes(const twv_griffin_lim* h);
/* Utterances of unequal lengths in one call: n_frames_host[b] >= 2 frames of utterance b (HOST int32, read here and not kept).
 * create's rules hold for every utterance (hop * (n_frames[b] - 1) > n_fft / 2); a violation is TWV_E_INVALID and the message
 * names the utterance's index.  Host work only.  Totals that do not fit hipFFT's `int` batch count are refused.
 * Packed layout of a ragged handle -- utterances concatenated, no padding rows:
 *   spec (total_frames, n_channels), uniforms (total_frames, n_fft/2+1), out (total_samples);
 *   utterance b owns frames [frame_offsets[b], frame_offsets[b+1]) and samples [sample_offsets[b], sample_offsets[b+1]),
 *   sample_offsets[b] = hop * (frame_offsets[b] - b): hop * (n_frames[b] - 1) samples each.
 * twv_inv_linear_spectrogram and twv_inv_spectrogram take a ragged handle with these layouts and are otherwise unchanged (every
 * norm_mode, the mel front, the [-1, 1] rule of preemphasis).  Overlap-add, reflect padding and the de-emphasis state stop at each
 * utterance's own ends: utterance b comes out as it does from a handle of its own.  The number of launches of a call depends
 * neither on batch nor on the lengths.  twv_griffin_lim_samples of a ragged handle is the LONGEST utterance's sample count;
 * workspace_bytes includes the per-utterance offset table the kernels read (copied into the workspace in stream order by each call). */
int twv_griffin_lim_create_ragged(int n_fft, int hop, int win_length, const int32_t* n_frames_host, int batch, twv_griffin_lim** out);
/* Sums over the batch; on a handle of twv_griffin_lim_create batch * n_frames and batch * samples. */
int64_t twv_griffin_lim_total_frames(const twv_griffin_lim* h);
int64_t twv_griffin_lim_total_samples(const twv_griffin_lim* h);
/* batch + 1 HOST entries each (the last ones are the totals); either pointer may be NULL.  A uniform handle answers b * n_frames
 * and b * samples. */
int twv_griffin_lim_offsets(const twv_griffin_lim* h, int64_t* frame_offsets_host, int64_t* sample_offsets_host);
/* lin (batch, n_frames, n_fft/2+1): the normalised linear spectrogram exactly as twv_tacotron_infer emits it; uniforms (same shape)
 * in [0,1) replace np.random.rand of utils/audio.py:131; out (batch, samples).  iters = hparams.griffin_lim_iters.
 * preemphasis = k of the inverse pre-emphasis lfilter([1], [1, -k]) (:27-30), 0 when hparams.preemphasize is off: computed as the
 * exact recurrence y[n] = x[n] + k*y[n-1] over the whole utterance (float32, the state carried across the kernel's chunks) for every
 * k in [-1, 1]; any other k (|k| > 1: an unstable filter; NaN) is TWV_E_INVALID before anything is launched -- in
 * twv_inv_spectrogram too. */
int twv_inv_linear_spectrogram(twv_griffin_lim* h, const float* lin, const float* uniforms, int iters, double power, double ref_level_db,
                               double max_abs_value, double min_level_db, double preemphasis, void* workspace, float* out, void* stream);
/* The same loop behind the general front of utils/audio.py:77-110.  spec (batch, n_frames, n_channels): n_channels = n_fft/2+1 with
 * inv_basis NULL is inv_linear_spectrogram (:77-92); n_channels = n_mels with a device inv_basis (n_fft/2+1, n_mels) row-major
 * (= np.linalg.pinv(mel basis)) is inv_mel_spectrogram (:95-110, _mel_to_linear :187-191: max(1e-10, inv_basis @ db_to_amp(D + ref))).
 * norm_mode selects _denormalize (:222-234): 0 none (signal_normalization off), 1 clip + symmetric (the hparams default),
 * 2 clip + asymmetric, 3 no clip + symmetric, 4 no clip + asymmetric.  uniforms (batch, n_frames, n_fft/2+1) in both cases. */
int twv_inv_spectrogram(twv_griffin_lim* h, const float* spec, int n_channels, const float* inv_basis, const float* uniforms,
                        int iters, double power, double ref_level_db, double max_abs_value, double min_level_db, int norm_mode,
                        double preemphasis, void* workspace, float* out, void* stream);

/* ======================================= waveform -> mel / linear spectrogram =======================================
 * utils/audio.py:61-75 `linearspectrogram` / `melspectrogram` for a ragged batch, both from one FFT pass:
 *   x = lfilter([1, -k], [1], wav) (:22-25);  D = librosa.stft(x, n_fft, hop, win_length) (:139-143: centre, reflect padding of
 *   n_fft/2, periodic Hann zero-padded to n_fft, 1 + len / hop frames);  A = |D| or mel_basis @ |D| (:181-185);
 *   S = 20 log10(max(min_level, A)) - ref_level_db, min_level = exp(min_level_db / 20 * ln 10) (:201-203);  _normalize(S) (:208-220).
 * mel_basis_host (n_mels, n_fft/2+1) row-major HOST floats = librosa.filters.mel(...) (:199), an input: the library computes no
 * basis.  Only each row's span first .. last non-zero is kept (a dense row keeps its whole width).  n_mels = 0: no mel output.
 * create does no device work (the basis is copied on the host and uploaded by the first analyze). */
typedef struct twv_spectrogram twv_spectrogram;
int twv_spectrogram_create(int n_fft, int hop, int win_length, int n_mels, const float* mel_basis_host, int max_samples, int batch,
                           twv_spectrogram** out);
void twv_spectrogram_destroy(twv_spectrogram* h);
int twv_spectrogram_frames(const twv_spectrogram* h);                  /* 1 + max_samples / hop: rows per utterance of the outputs */
size_t twv_spectrogram_workspace_bytes(const twv_spectrogram* h);
/* wav (batch, max_samples) device; lengths_host[batch] (HOST; NULL = every utterance has max_samples), each n_fft/2 < len <=
 * max_samples.  mel_out (batch, frames, n_mels) and lin_out (batch, frames, n_fft/2+1), device, either may be NULL; rows past an
 * utterance's 1 + len / hop frames are 0.  preemphasis = 0 when hparams.preemphasize is off.  norm_mode: 0 none, 1 clip +
 * symmetric, 2 clip + asymmetric, 3 no clip + symmetric, 4 no clip + asymmetric (_normalize, :208-220).  minmax_out (device
 * float[2], or NULL): min and max of S over every value written, for the assertion of :216 that the no-clip modes carry. */
int twv_spectrogram_analyze(twv_spectrogram* h, const float* wav, const int32_t* lengths_host, double preemphasis, double ref_level_db,
                            double min_level_db, double max_abs_value, int norm_mode, void* workspace, float* mel_out, float* lin_out,
                            float* minmax_out, void* stream);

/* ======================================= resampling (any wav rate -> the model's) =======================================
 * utils/audio.py:11-12 `librosa.core.load(path, sr=sr)` (and generate.py:90 for --wav_seed): channels averaged, then a band-limited
 * rational resampler, for a ragged batch.  The arithmetic is this project's contract ("Resampling"):
 *   g = gcd(sr_in, sr_out), L = sr_out / g, M = sr_in / g, s = min(1, L / M);  n_out = ceil(n_in * L / M) in integers;
 *   y[t] = sum_n x[n] * s * h(s * (t * M / L - n)), x zero outside [0, n_in), position exact: q = (t M) div L, p = (t M) mod L;
 *   h(u) = r sinc(r u) I0(beta sqrt(1 - (u / Z)^2)) / I0(beta) for |u| < Z, else 0;
 *   Z = 64, r = 0.9475937167399596, beta = 14.769656459379492   [RECALLED: resampy's kaiser_best; unpinned against librosa].
 * create does host work only: the L x taps table c[p][k] = s h(s (k - taps/2 + p / L)), y[t] = sum_k c[p][k] x[q + taps/2 - k],
 * taps = 2 * (ceil(Z / s) rounded up to a multiple of 4), computed in double and rounded once to float32.  It refuses rates <= 0,
 * equal rates (TWV_E_INVALID) and, with TWV_E_UNSUPPORTED, a ratio whose table exceeds 2^20 floats (every pair among 8000, 11025,
 * 16000, 22050, 24000, 32000, 44100, 48000, 96000 Hz is far below: at most 1280 x 128, or 147 x 1120) or whose tile does not fit LDS. */
typedef struct twv_resampler twv_resampler;
int twv_resample_create(int sr_in, int sr_out, int max_samples_in, int batch, twv_resampler** out);
void twv_resample_destroy(twv_resampler* h);
int twv_resample_phases(const twv_resampler* h);                        /* L */
int twv_resample_taps(const twv_resampler* h);                          /* columns of the table */
int64_t twv_resample_out_samples(const twv_resampler* h, int64_t n_in); /* ceil(n_in * L / M); -1 for a negative n_in */
size_t twv_resample_workspace_bytes(const twv_resampler* h);
int twv_resample_filter_host(const twv_resampler* h, float* out);       /* HOST float[phases * taps]: the table, row-major */
const char* twv_resample_kernel_name(const twv_resampler* h);           /* which instantiation twv_resample launches (the handle owns it) */
int twv_resample_rounds(const twv_resampler* h);                        /* rounds per workgroup: a tile is phases * rounds outputs */
/* in (batch, max_samples_in[, channels]) device: in_format 0 = float32, 1 = int16 (scaled by 1 / 32768); channels 1, or 2 interleaved
 * and averaged (librosa.load's mono=True) -- both happen while the input is staged, there is no separate pass.  lengths_host[batch]
 * (HOST; NULL = every utterance has max_samples_in), 0 <= len <= max_samples_in.  out (batch, out_samples(max_samples_in)) float32
 * device; a row is 0 past its utterance's out_samples(len).  workspace: workspace_bytes of device memory, 256-byte aligned, that
 * belongs to the handle between calls (the table is uploaded into a workspace the handle sees for the first time). */
int twv_resample(twv_resampler* h, const void* in, int in_format, int channels, const int32_t* lengths_host, void* workspace, float* out,
                 void* stream);

/* cross-lane primitive self-test (device float[256]); used by the gpu tests to pin v_permlane32_swap / v_readlane semantics */
int twv_selftest(float* out256, void* stream);
/* test aid: `blocks` workgroups that each hold `lds_bytes` of LDS and spin for `milliseconds` on `stream` -- stands in for "another
 * kernel is using the device" in the co-residency test of the persistent generation kernel (TWV_E_BUSY). */
int twv_debug_occupy(int blocks, int lds_bytes, double milliseconds, void* stream);

/* ---- checkpoint helper (host only) ----
 * CRC-32C of `n` bytes, continuing from `crc` (0 to start): the per-tensor / per-block checksum of the TensorFlow
 * tensor-bundle files that tf.train.Saver writes (train_vocoder.py:133,176 / generate.py:158-161); used by
 * checkpoint.py to verify bundles on read and to stamp the ones it writes.  No device work. */
uint32_t twv_crc32c(const void* data, size_t n, uint32_t crc);

#ifdef __cplusplus
}
#endif
#endif
