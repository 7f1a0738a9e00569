/*
 * nww.h - C-ABI of libnwwhip.so: the MI355X (gfx950) implementation of nanowakeword's
 * batched keyword-spotting hot path  int16 PCM -> STFT -> mel -> dB -> classifier head -> logit.
 *
 * The reference (arcosoph/nanowakeword v3.0.0) is pure Python and has no FFI of its own; its
 * hot path sits behind a duck-typed onnxruntime.InferenceSession:
 *     session.get_inputs()[0].{name,shape}        nanointerpreter.py:165-167,177-178
 *     session.run(None, {"input": x}) -> [probs(B,1,1)]   nanointerpreter.py:677,681,783
 * with `_RemoteSession` (remote_verifier.py:490-648) as the in-tree precedent of a non-ORT
 * backend.  This header is what a ctypes binding of such a backend binds;
 * nanowakeword_amd/session.py is that binding.
 *
 * Conventions: extern "C", opaque handle, int return codes (0 = ok), no exceptions or C++ types
 * across the boundary.  Buffers are caller-owned.  `*_host` entry points take host pointers and
 * synchronise before returning; `*_dev` entry points take device pointers, enqueue on the given
 * hipStream_t (NULL = the handle's own stream) and do NOT synchronise.  A handle is bound to one
 * GPU and is not re-entrant (the reference interpreter is single-threaded too:
 * nanointerpreter.py:955-959); use one handle per GPU / per thread.
 */
#ifndef NWW_H
#define NWW_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NWW_OK 0
#define NWW_ERR_INVALID 1      /* bad argument (ValueError in the reference's terms)          */
#define NWW_ERR_MISSING 2      /* finalize(): a state_dict tensor was never loaded            */
#define NWW_ERR_SHAPE 3        /* load_tensor(): shape differs from Model.state_dict()        */
#define NWW_ERR_HIP 4          /* a HIP runtime call failed; see nww_last_error               */
#define NWW_ERR_STATE 5        /* call order: run before finalize, load after finalize        */
#define NWW_ERR_UNSUPPORTED 6

/* head_type: which nanowakeword/modules/architectures.py class the handle evaluates */
#define NWW_HEAD_DNN 0         /* Net                     architectures.py:102-126 */
#define NWW_HEAD_CNN 1         /* CNNModel                architectures.py:51-80   */
#define NWW_HEAD_CRNN 2        /* CRNNModel (rnn=gru)     architectures.py:209-287 */
#define NWW_HEAD_GRU 3         /* GRUModel                architectures.py:129-145 */
#define NWW_HEAD_BCRESNET 4    /* BcResNetModel           architectures.py:620-687 */
#define NWW_HEAD_CONFORMER 5   /* ConformerModel          architectures.py:441-543 */
#define NWW_HEAD_E2E_DNN 6     /* E2E_MelSpectrogram_CNN  architectures.py:820-889 */
#define NWW_HEAD_TRANSFORMER 7 /* TransformerModel        architectures.py:164-206 */
#define NWW_HEAD_TCN 8         /* TCNModel                architectures.py:290-367 */
#define NWW_HEAD_E_BRANCHFORMER 9 /* EBranchformerModel   architectures.py:546-616 */
#define NWW_HEAD_QUARTZNET 10  /* QuartzNetModel          architectures.py:370-437 */
#define NWW_HEAD_E2E_QUARTZNET 11 /* E2ERawQuartzNet      architectures.py:798-817; model.py:119-132 (learned filters on raw PCM, no STFT) */
#define NWW_HEAD_RNN 12        /* RNNModel (bi-LSTM, hidden size 64; layer_dim is not read)  architectures.py:149-161 */
#define NWW_HEAD_E2E_CNN 13    /* E2ERawCNN               architectures.py:739-795; model.py:109-117 (the raw-PCM frontend, then strided 3x3 convs) */

#define NWW_ACT_RELU 0         /* model.py:81-87 activation_function */
#define NWW_ACT_GELU 1
#define NWW_ACT_SILU 2

#define NWW_DTYPE_F32 0

typedef struct nww_handle nww_handle;

typedef struct nww_config {
    int32_t device;            /* HIP device ordinal                                          */
    /* frontend: T.MelSpectrogram(...) + T.AmplitudeToDB() of architectures.py:830-837,
       evaluated as the exported ONNXSafeMelSpectrogram (_export/onnx.py:27-83)               */
    int32_t sample_rate;       /* 16000                                                       */
    int32_t n_fft;             /* 400 (only 400 = 8*25*2 is implemented)                      */
    int32_t win_length;        /* 400                                                         */
    int32_t hop_length;        /* 160                                                         */
    int32_t n_mels;            /* <= 128                                                      */
    int32_t center;            /* 1: reflect-pad n_fft/2 (reference e2e), 0: no padding       */
    float f_min, f_max;        /* 0, sample_rate/2                                            */
    float amin;                /* 1e-10 clamp floor (-100 dB)                                 */
    float db_multiplier;       /* 10 (power spectrogram)                                      */
    /* head: kwargs/config keys of Model() (model.py:67-296)                                  */
    int32_t head_type;         /* NWW_HEAD_*                                                  */
    int32_t in_rows, in_cols;  /* Model(input_shape=(in_rows, in_cols))                       */
    /* NWW_HEAD_E2E_QUARTZNET: layer_dim carries e2e_frontend_channels and n_blocks e2e_frontend_depth (1..4; E2ERawQuartzNet reads
       neither, as TCNModel reads no layer_dim); in_cols = layer_dim << (n_blocks - 1) (<= 512) is what its QuartzNet backbone sees,
       in_rows the raw frontend's rows for the clip length: per stage L' = (L - 1) / stride + 1 with strides 16, 4, 4, ...; its
       e2e_quartznet_config travels as NWW_HEAD_QUARTZNET's entries do; mel_major_features = 0 and the mel fields are ignored.
       For this head nww_num_frames is that frame law, nww_frontend* return the learned frontend's output ([B][in_cols][rows], or
       [B][rows][in_cols] with frames_major; melpower_out must be NULL), nww_forward_features* run the backbone alone.
       NWW_HEAD_E2E_CNN: the same frontend fields (its depth defaults to 2 in the reference); the backbone's channel counts are fixed by
       the architecture, the image it sees is in_cols high and in_rows wide */
    int32_t layer_dim, n_blocks, embedding_dim, activation;
    /* crnn_cnn_channels (<= 4 stages) for NWW_HEAD_CRNN; tcn_channels (1..4 levels, model.py:228) for NWW_HEAD_TCN, whose
       tcn_kernel_size (>= 2) travels in layer_dim (TCNModel reads no layer_dim); quartznet_config (model.py:239-248) for
       NWW_HEAD_QUARTZNET: n_crnn_channels = its number of [channels, kernel, repetitions] entries (1..4), crnn_channels[i] = entry
       i's channels, quartznet_kr[i] (below) = its kernel + 65536 * its repetitions.  More than 4 entries, or more than 16 blocks
       once the repetitions are expanded, is NWW_ERR_UNSUPPORTED at nww_create                                          */
    int32_t n_crnn_channels;
    int32_t crnn_channels[4];
    /* d_model / n_head of the attention encoder (Conformer, Transformer, E-Branchformer): conformer_d_model / conformer_n_head
       for NWW_HEAD_CONFORMER, transformer_d_model / transformer_n_head (model.py:200-201) for NWW_HEAD_TRANSFORMER,
       branchformer_d_model / branchformer_n_head (model.py:263-274) for NWW_HEAD_E_BRANCHFORMER                          */
    int32_t conformer_d_model, conformer_n_head;
    /* how nww_forward_pcm feeds the head: 0 = log-mel transposed to (frames, n_mels) =
       Model(input_shape=(frames, n_mels)); 1 = (n_mels, frames) as E2E_MelSpectrogram_CNN.   */
    int32_t mel_major_features;
    /* arithmetic of the large MFMA contractions - conv2 of the fused conv trunk (CNN / CRNN / E2E heads) and Linear
       layers with K >= 4096 (fc1 of the CNN head); every mode computes float32 results from float32 data, they differ
       in how the products are formed:
         NWW_ARITH_F32    v_mfma_f32_32x32x2_f32, one fmaf chain per output
         NWW_ARITH_BF16X9 each float32 operand split into three bf16 terms (exact), all nine partial products on
                          v_mfma_f32_32x32x16_bf16 - exact products, float32 accumulation
         NWW_ARITH_BF16X6 the six largest partial products; the dropped ones are < 2^-23 of a product
         NWW_ARITH_F16X3  each operand, scaled by a power of two fixed at nww_finalize from bounds on the tensors (features
                          are clamped to +-NWW_F16_FEATURE_BOUND = 8192: log-mel dB values lie in [-100, 60]; the accuracy does not depend on how generous the bound is), split into TWO
                          binary16 terms holding 22-23 of its 24 significant bits; the three partial products >= 2^-22 of a
                          product on v_mfma_f32_32x32x16_f16, float32 accumulation - half the matrix instructions of
                          BF16X6 at the float32 MFMA's accuracy against float64.  Layers without an f16x3 instance, or
                          without a bound on their input, run as NWW_ARITH_BF16X6
         NWW_ARITH_DEFAULT lets the library choose: NWW_ARITH_F16X3 (nww_api.hip NWW_DEFAULT_CONV_ARITH).  Under it the
                          head input is clamped to +-NWW_F16_FEATURE_BOUND - also for nww_forward_features* callers whose
                          features are not log-mel dB (the reference applies no clamp: pass NWW_ARITH_BF16X6 for
                          unbounded features)                                                                    */
    int32_t conv_arith;
    /* recurrent backend of the CRNN head: 0 = GRU, 1 = LSTM (the reference's default, modules/model.py:214;
       CRNNModel, modules/architectures.py:238-254)                                                               */
    int32_t crnn_rnn_lstm;
    /* storage type of the activation tensors BETWEEN the head's kernels: NWW_ACT_DTYPE_F32 (default), NWW_ACT_DTYPE_BF16 (round to
       nearest even on store; products and accumulation stay float32) or NWW_ACT_DTYPE_F16 (binary16 of value x a power of two
       fixed per tensor at plan time from a bound on it, round to nearest even, saturating; same bytes and speed as bf16, 11
       significant bits instead of 8).  Both are opt-ins for the BcResNet head (BASELINE.json config 3 "bf16 activations"):
       bf16 logits agree with the float32 reference to ~2e-2 on the test clips except all-zero PCM (0.2); f16 logits to ~5e-3 on
       every clip.  f16 assumes features within +-NWW_F16_FEATURE_BOUND, like NWW_ARITH_F16X3.                               */
    int32_t act_dtype;
    /* NWW_HEAD_QUARTZNET: kernel + 65536 * repetitions of quartznet_config entry i (kernel 1..65535, repetitions >= 1); zero and
       ignored for every other head (these were the four reserved words: the struct keeps its 132 bytes and every offset)    */
    int32_t quartznet_kr[4];
} nww_config;
#define NWW_ACT_DTYPE_F32 0
#define NWW_ACT_DTYPE_BF16 1
#define NWW_ACT_DTYPE_F16 2
#define NWW_ARITH_DEFAULT 0
#define NWW_ARITH_F32 1
#define NWW_ARITH_F16X3 3
#define NWW_F16_FEATURE_BOUND 8192.0f
#define NWW_ARITH_BF16X6 6
#define NWW_ARITH_BF16X9 9

/* Fill *cfg with the reference defaults (16 kHz, 400/400/160, 64 mel, center, DNN (16,96)). */
void nww_default_config(nww_config* cfg);

int nww_create(const nww_config* cfg, nww_handle** out);
int nww_destroy(nww_handle* h);
const char* nww_last_error(const nww_handle* h);   /* h may be NULL: last create() error      */

/* Weights. `key` is exactly a Model.state_dict() key ("model.conv1.weight", "classifier.0.bias",
 * BatchNorm "running_mean"/"running_var"; "num_batches_tracked" is accepted and ignored).
 * Optional frontend tables taken from an exported model instead of the built-in torchaudio
 * formulas: "frontend.window" [win_length] and "frontend.mel_fb" [n_fft/2+1, n_mels]
 * (ONNXSafeMelSpectrogram buffers real_basis[0,0,:] and mel_fb, _export/onnx.py:62-64).     */
int nww_load_tensor(nww_handle* h, const char* key, const void* host_data,
                    const int64_t* shape, int32_t ndim, int32_t dtype);
/* Number of tensors finalize() requires, and the i-th key/shape (for loaders/validators).    */
int nww_num_tensors(const nww_handle* h);
int nww_tensor_info(const nww_handle* h, int32_t i, const char** key, int64_t* shape4, int32_t* ndim);
/* Check completeness, fold BatchNorm (alpha = w/sqrt(var+eps), beta = b - mean*alpha, as
 * PyTorch's eval kernel), build FFT/mel tables, upload.                                      */
int nww_finalize(nww_handle* h);

/* Frame law (bit-exact): center ? 1 + N/hop : 1 + (N - n_fft)/hop ; <0 if N is too short.    */
int32_t nww_num_frames(const nww_handle* h, int32_t n_samples);

/* ---- host-pointer entry points (synchronous) --------------------------------------------- */
/* pcm [B,N] int16 -> logmel [B, n_mels, frames] float32 dB (the mel module's own layout).    */
int nww_frontend(nww_handle* h, const int16_t* pcm, int32_t B, int32_t N,
                 float* logmel_out, int32_t* frames_out);
/* same, additionally returning the mel power spectrogram [B, n_mels, frames] (may be NULL).  */
int nww_frontend_ex(nww_handle* h, const int16_t* pcm, int32_t B, int32_t N,
                    float* logmel_out, float* melpower_out, int32_t* frames_out);
/* pcm [B,N] -> logits [B] (Model.forward) and/or probs [B] (InferenceWrapper sigmoid,
 * _export/onnx.py:164-172).  Either output may be NULL.                                      */
int nww_forward_pcm(nww_handle* h, const int16_t* pcm, int32_t B, int32_t N,
                    float* logits, float* probs);
/* feats [B, in_rows, in_cols] float32 -> logits/probs; embedding [B, embedding_dim] optional. */
int nww_forward_features(nww_handle* h, const float* feats, int32_t B,
                         float* logits, float* probs);
int nww_forward_features_ex(nww_handle* h, const float* feats, int32_t B,
                            float* logits, float* probs, float* embedding);

/* ---- device-pointer entry points (asynchronous on `stream`, a hipStream_t) ----------------- */
int nww_frontend_dev(nww_handle* h, const int16_t* d_pcm, int32_t B, int32_t N,
                     float* d_logmel, int32_t frames_major, void* stream);
int nww_forward_pcm_dev(nww_handle* h, const int16_t* d_pcm, int32_t B, int32_t N,
                        float* d_logits, float* d_probs, void* stream);
int nww_forward_features_dev(nww_handle* h, const float* d_feats, int32_t B,
                             float* d_logits, float* d_probs, void* stream);
/* Pre-size the workspace for batches up to B clips of N samples (otherwise grown on demand,
 * which synchronises the device).                                                           */
int nww_reserve(nww_handle* h, int32_t B, int32_t N);

/* Names of the launches a forward_pcm performs, in order, one per line (rocprof correlation).  */
int nww_describe_plan(const nww_handle* h, char* buf, int32_t buflen);
/* The bound the finalized plan ASSUMES on the head's input features: +-NWW_F16_FEATURE_BOUND when a layer that reads them runs in the
   two-term binary16 arithmetic or 16-bit storage (values beyond it are clamped - the reference does not clamp), 0 when nothing is
   clamped.  Log-mel dB from nww_forward_pcm* always lies inside it; nww_forward_features* callers with other features can check:
   the Python host layer warns when a host feature array exceeds it.                                                              */
float nww_feature_clamp(const nww_handle* h);
/* Per-launch timing with HIP events ON THE STREAM THE KERNELS RUN ON.  While enabled, every
 * forward records one event per launch boundary (frontend, each head launch, sigmoid).
 * nww_get_profile synchronises those events and returns, per plan entry (same order as
 * nww_describe_plan), the accumulated milliseconds and the number of launches since the last
 * nww_set_profiling(h, 1).  n_inout: capacity in, entries out.  enable = n > 1 samples every n-th
 * forward only (each event costs the stream ~10 us; sampling keeps a timed loop undisturbed).    */
int nww_set_profiling(nww_handle* h, int32_t enable);
int nww_get_profile(nww_handle* h, float* ms_total, int32_t* launches, int32_t* n_inout);

/* ---- batched streaming (the front half of NanoInterpreter.predict in E2E mode, for S lock-step streams) ----
 * Replaces, per stream, the deque(maxlen=clip_samples) + "last clip_samples" window of
 * nanointerpreter.py:181,746-756 with a device-resident ring (double-written so the last `window` samples
 * are always contiguous).  Every push appends `hop` new samples per stream and re-scores the whole window,
 * exactly as the reference recomputes its window on every predict() call.  Scores are 0 until a stream has
 * seen `window` samples (nanointerpreter.py:755,785-786).  Post-filters stay on the host (a18).            */
int nww_stream_open(nww_handle* h, int32_t n_streams, int32_t window_samples, int32_t hop_samples);
/* chunk [n_streams][hop] int16 (host pointer); logits/probs [n_streams] host, either may be NULL.         */
int nww_stream_push(nww_handle* h, const int16_t* chunk, float* logits, float* probs);
/* device variant: d_chunk [n_streams][hop], outputs device pointers, enqueued on `stream`, no sync.       */
int nww_stream_push_dev(nww_handle* h, const int16_t* d_chunk, float* d_logits, float* d_probs, void* stream);
int nww_stream_reset(nww_handle* h);      /* new session for every stream (NanoInterpreter.reset, :719-733)    */
int nww_stream_close(nww_handle* h);
/* samples seen per stream since open/reset (of a batch whose streams share one state; nww_stream_filled_of otherwise) */
int64_t nww_stream_filled(const nww_handle* h);

/* ---- streams that push, join and reset on their own: the serving shape of the batch above ----
 * The same open batch, every stream with a write position, fill count and log-mel ring rotation of its own, kept on the host (every
 * push is commanded by the host: no device counter, no read-back); a call uploads one small table for its listed streams.  A client
 * that connects takes a free stream through nww_stream_reset_some and inherits nothing; a client whose packet is late is left out of
 * the tick.  Every score is bit-identical to nww_forward_pcm on the scored streams' last `window` samples stacked in idx order.
 * Route 1 (shared frames), where nww_stream_push keeps a log-mel ring for a mel head: the scored windows are gathered out of the PCM
 * rings, the frontend computes for a stream whose ring holds its previous window only the frames the hop invalidates (12 of 101 at
 * 1 s / 80 ms), for a stream's first full window all of them; the rows are placed in each stream's own ring and each window gathered
 * from its own rotation into the dense head input.  Route 0 (whole windows) otherwise - a raw-PCM head, a hop that is no multiple of
 * hop_length, NWW_STREAM_INC=0, a frontend without frame subsets: nww_forward_pcm's own path on the gathered windows.
 * While every stream shares one state (a fresh or reset batch, and as long as every call lists every stream) the batch is ALIGNED and
 * nww_stream_push* / nww_cascade_stream_push* work as before; the first push_some / reset_some that makes the states differ ends
 * that, and those lock-step calls return NWW_ERR_STATE until nww_stream_reset.  A cascade does not need lock-step:
 * nww_cascade_stream_push_some / nww_cascade_stream_reset_some (the cascade block below) run a gate + verifier pair on a batch in any
 * state.  The pooled conv rows and sequence rows nww_stream_push keeps for the CRNN stem are not kept per stream.
 * (Declared `extern` like the recording block below: the pinned count of declarations that start a line with their return type
 * stays 48.)                                                                                                                        */
/* idx: HOST pointer, n strictly ascending stream numbers in [0, n_streams).  chunk [n][hop]: row i belongs to stream idx[i].  Outputs
 * [n], in idx order (either may be NULL); a stream whose own ring does not yet hold a window gets 0 (logit and probability).  n == 0 is
 * NWW_OK and launches nothing.  idx not strictly ascending or out of range: NWW_ERR_INVALID, and nothing is written.                */
extern int nww_stream_push_some(nww_handle* h, const int32_t* idx, int32_t n, const int16_t* chunk, float* logits, float* probs);
/* device variant: d_chunk and the outputs are device pointers (idx stays a host pointer), enqueued on `stream`, no sync.  A d_chunk
 * that is 16-byte aligned is copied 16 bytes per thread.                                                                          */
extern int nww_stream_push_some_dev(nww_handle* h, const int32_t* idx, int32_t n, const int16_t* d_chunk, float* d_logits, float* d_probs, void* stream);
/* New session for the listed streams only: their PCM rings are zeroed, their fill counts are 0 and their next full window is
 * computed whole.  Synchronises the device.                                                                                       */
extern int nww_stream_reset_some(nww_handle* h, const int32_t* idx, int32_t n);
/* samples seen by one stream since open / its last reset                                                                          */
extern int64_t nww_stream_filled_of(const nww_handle* h, int32_t stream);
/* Test and tool instrument, for the latest push_some: how many streams were scored, the route taken (1 shared frames, 0 whole
 * windows) and how many log-mel frames (rows of a raw-PCM frontend) the frontend was asked for in total.  Outputs may be NULL.      */
extern int nww_stream_pool_stats(const nww_handle* h, int32_t* n_scored, int32_t* route, int64_t* frames_computed);

/* ---- recording scoring: every window of ONE long recording in a call (the offline counterpart of nww_stream_*) ----
 * What NanoInterpreter.predict computes chunk after chunk over a file (test_model/evaluate_model_with_audio.py), as batches: window i
 * is pcm[i * hop, i * hop + window), i = 0 .. nW - 1, nW = 1 + (n_samples - window) / hop (a trailing partial hop is ignored).  The
 * recording is read where it lies (row_stride = hop): nothing is cut into windows, on the host or on the device.  Every logit is
 * bit-identical to nww_forward_pcm on the same windows in batches of the passes' sizes.  window and hop: positive multiples of 8
 * samples, hop <= window (NWW_ERR_INVALID), and the window must give the head's (in_rows, in_cols) (NWW_ERR_SHAPE) - the rules of
 * nww_stream_open.  An offset of the first window is the caller's pointer arithmetic (pcm + offset).
 * Two routes: shared frames - a pass computes every interior log-mel frame once, the frames of each window that
 * touch its own reflect padding apart, and assembles the windows on the device - when hop is a multiple of hop_length, the head
 * reads frames-major log-mel and NWW_REC_SHARED is not 0; otherwise the strided route, which recomputes every window's frames.
 * The raw-PCM heads (e2e_quartznet, e2e_cnn) share the rows of their learned frontend's last stage in the same way - the pool is
 * the one-launch frontend over the pass's span, a row-subset instance of it computes the rows of each window that see its own zero
 * padding - when that frontend is planned (depth 2 or 3, 16 or 32 channels, NWW_RAW_FUSED not 0) and hop is a multiple of the
 * frontend's total stride 16 * 4^(depth - 1); nww_stream_push keeps a ring of those rows under the same rule (NWW_STREAM_INC).
 * (The five - nww_recording_poison included - are declared `extern`, which changes nothing for a C compiler: tests/test_e2e_cnn_head.py and test_e2e_quartznet_head.py
 * count the declarations that start a line with their return type, and that count - 48 - is the one they pin.)                          */
/* nW for n_samples (0: shorter than one window); < 0: minus the error code, text in nww_last_error                                  */
extern int nww_recording_windows(nww_handle* h, int32_t n_samples, int32_t window, int32_t hop);
/* 1: shared-frame route, 0: strided route, < 0: minus the error code                                                                */
extern int nww_recording_route(nww_handle* h, int32_t window, int32_t hop);
/* d_pcm [n_samples] int16 -> d_logits / d_probs [nW] (either may be NULL), in passes of at most max_batch windows (<= 0: 4096);
 * asynchronous on `stream`.  The workspace is that of nww_reserve(max_batch, window) plus the pass's frame pool; it grows on the
 * first call of a size (which synchronises the device).                                                                            */
extern int nww_forward_recording_dev(nww_handle* h, const int16_t* d_pcm, int32_t n_samples, int32_t window, int32_t hop, int32_t max_batch,
                              float* d_logits, float* d_probs, void* stream);
/* host pointers; the recording is uploaded once (2 bytes per sample, in pieces), never as windows.  n_windows_out may be NULL.      */
extern int nww_forward_recording(nww_handle* h, const int16_t* pcm, int32_t n_samples, int32_t window, int32_t hop, int32_t max_batch,
                          float* logits, float* probs, int32_t* n_windows_out);
/* test instrument: fills the shared route's pool and the dense head input with `value` (synchronises), so that a later pass which
 * left one of their rows unwritten cannot score as before                                                                            */
extern int nww_recording_poison(nww_handle* h, float value);

/* ---- gate + verifier cascades: the verifier runs on the windows the gate opens (NanoInterpreter.load_model(cascade=True)) ----
 * Two finalized handles on one device, a small gate and the verifier, and a threshold.  The gate scores every window; a window is
 * CLOSED exactly when (double)gate_prob < gate_threshold (nanointerpreter.py:660-669, 758-769 on float(np.float32): a NaN probability
 * leaves the window open, a threshold <= 0 opens all, one > 1 closes all); the open windows' indices are compacted on the device in
 * ascending order (block counts, a prefix sum, a placement pass: no atomic counter), their samples gathered into the verifier's PCM
 * staging, the verifier run by nww_forward_pcm's own path on consecutive chunks of at most max_batch survivors (the batch entry point
 * and the stream push: all survivors of the call as one batch), and its outputs scattered back.  Outputs are dense, one per window:
 * the gate's probabilities bit-identical to the gate handle alone on the same input, the verifier's logits / probabilities
 * bit-identical to nww_forward_pcm on the open windows stacked in ascending order in those chunks, and 0.0f / -INFINITY on closed
 * windows.  With no window open the verifier is not launched.  The two handles may differ in everything but the device; the window
 * must give each its own (in_rows, in_cols) (NWW_ERR_SHAPE, the text naming which of the two).  Handles that are not finalized, not
 * distinct or on two devices: NWW_ERR_INVALID.  Errors go to nww_last_error(verifier); the index list, the dense outputs of the
 * host-pointer variants and the pinned count live on the verifier's handle and grow on demand.
 * The count of open windows is read back through one pinned 4-byte copy: every entry point synchronises `stream` ONCE, behind the
 * gate's last pass and the select (never once per pass), and checks 0 <= n_open <= n before it sizes anything (NWW_ERR_HIP
 * otherwise).  The verifier's launches are asynchronous on `stream` in the _dev variants; the host-pointer variants synchronise a
 * second time before they return.  stream NULL: the verifier's own stream.  n_open_out may be NULL.  DESIGN.md 4.8c.
 * (Declared `extern` like the recording block above: the pinned count of declarations that start a line with their return type
 * stays 48.)                                                                                                                        */
/* The select alone, on the caller's scores: probs [n] host -> idx_out [n_open] host (room for n entries), ascending.                  */
extern int nww_cascade_select(nww_handle* verifier, const float* probs, int32_t n, double gate_threshold, int32_t* idx_out, int32_t* n_open_out);
/* d_pcm [B][N] -> d_gate_probs / d_logits / d_probs [B] (d_gate_probs may be NULL; d_logits or d_probs may be NULL)                    */
extern int nww_cascade_forward_pcm_dev(nww_handle* gate, nww_handle* verifier, const int16_t* d_pcm, int32_t B, int32_t N, double gate_threshold,
                                float* d_gate_probs, float* d_logits, float* d_probs, int32_t* n_open_out, void* stream);
extern int nww_cascade_forward_pcm(nww_handle* gate, nww_handle* verifier, const int16_t* pcm, int32_t B, int32_t N, double gate_threshold,
                            float* gate_probs, float* logits, float* probs, int32_t* n_open_out);
/* every window of a recording (the rules of nww_forward_recording*): the gate scores ALL passes first, on whichever route it plans,
 * then one select over the nW windows, then the verifier's chunks, gathered from the recording where it lies (row_stride = hop)      */
extern int nww_cascade_forward_recording_dev(nww_handle* gate, nww_handle* verifier, const int16_t* d_pcm, int32_t n_samples, int32_t window, int32_t hop,
                                      int32_t max_batch, double gate_threshold, float* d_gate_probs, float* d_logits, float* d_probs,
                                      int32_t* n_open_out, void* stream);
/* host pointers; the recording is uploaded once, as nww_forward_recording does.  n_windows_out may be NULL.                           */
extern int nww_cascade_forward_recording(nww_handle* gate, nww_handle* verifier, const int16_t* pcm, int32_t n_samples, int32_t window, int32_t hop,
                                  int32_t max_batch, double gate_threshold, float* gate_probs, float* logits, float* probs,
                                  int32_t* n_windows_out, int32_t* n_open_out);
/* S lock-step streams: only the GATE has a stream open (nww_stream_open on it, at whatever incremental level it plans); the verifier
 * keeps no ring and scores the full windows of the open streams out of the gate's PCM ring.  Until the ring holds a window every
 * output is 0 and the verifier is not run, as in nww_stream_push.  chunk [S][hop]; outputs [S].                                       */
extern int nww_cascade_stream_push(nww_handle* gate, nww_handle* verifier, const int16_t* chunk, double gate_threshold, float* gate_probs,
                            float* logits, float* probs, int32_t* n_open_out);
extern int nww_cascade_stream_push_dev(nww_handle* gate, nww_handle* verifier, const int16_t* d_chunk, double gate_threshold, float* d_gate_probs,
                                float* d_logits, float* d_probs, int32_t* n_open_out, void* stream);
/* The listed streams of a batch whose streams push, join and reset on their own (nww_stream_push_some): the gate's
 * batch may be in any state, aligned or not.  idx and chunk follow nww_stream_push_some: idx a HOST pointer to n strictly ascending
 * stream numbers, chunk [n][hop] with row i for stream idx[i]; only the gate has a stream batch open.  Outputs [n], in idx order, any of
 * them NULL under the rules of nww_cascade_stream_push*:
 *     the stream's own ring holds no window yet    gate_probs 0             logits 0            probs 0
 *     scored, closed                               the gate alone           -INFINITY           0.0f
 *     scored, open                                 the gate alone           the verifier        the verifier
 * gate_probs[i] is bit-identical to what nww_stream_push_some on the gate alone writes for the same call.  A stream that holds no
 * window is never open, whatever the threshold: gate_threshold <= 0 opens every SCORED stream.  The open streams' outputs are
 * bit-identical to nww_forward_pcm on the verifier for those streams' last `window` samples, stacked in ascending stream order as ONE
 * batch.  *n_open_out: the open streams; with none the verifier launches nothing.  The open entries are compacted by a select that walks
 * the call's table on the device (count, prefix sum, placement: ascending, no atomic counter) and leaves each open stream's window
 * offset in the gate's PCM rings for the gather and its output index for the scatter.
 * n == 0: NWW_OK, nothing is launched, *n_open_out = 0.  Every check that needs no device runs BEFORE the gate's push touches a ring,
 * so a call that fails one leaves every nww_stream_filled_of as it was: the handles distinct, finalized and on one device
 * (NWW_ERR_INVALID), the gate with an open batch (NWW_ERR_STATE), idx valid (NWW_ERR_INVALID), the window giving the verifier its
 * (in_rows, in_cols) (NWW_ERR_SHAPE, the text naming the verifier).  A failure BEHIND the gate's push - a launch, the count's
 * read-back, the verifier's workspace - leaves the gate's listed streams advanced by the hop, as nww_cascade_stream_push leaves them.
 * Synchronisation as above: `stream` once, behind the gate and the select, for the pinned 4-byte count (not at all when no listed
 * stream holds a window), 0 <= n_open <= n checked before anything is sized; the host-pointer variant a second time before it returns.
 * A call that lists every stream of an aligned batch keeps it aligned, and nww_cascade_stream_push* runs afterwards.                 */
extern int nww_cascade_stream_push_some(nww_handle* gate, nww_handle* verifier, const int32_t* idx, int32_t n, const int16_t* chunk,
                                 double gate_threshold, float* gate_probs, float* logits, float* probs, int32_t* n_open_out);
/* device variant: d_chunk and the outputs are device pointers, idx stays a host pointer (as in nww_stream_push_some_dev)             */
extern int nww_cascade_stream_push_some_dev(nww_handle* gate, nww_handle* verifier, const int32_t* idx, int32_t n, const int16_t* d_chunk,
                                     double gate_threshold, float* d_gate_probs, float* d_logits, float* d_probs, int32_t* n_open_out,
                                     void* stream);
/* the gate's nww_stream_reset_some (the verifier keeps no ring); its errors are reported on the verifier's handle                  */
extern int nww_cascade_stream_reset_some(nww_handle* gate, nww_handle* verifier, const int32_t* idx, int32_t n);

/* ---- model banks: several wake words on ONE frontend pass (NanoInterpreter scores every loaded model on the same audio) ----
 * A bank is k >= 1 finalized handles on one device whose mel frontends are identical.  It is not an object: like a cascade it is the
 * list of handles passed with each call.  members[0] is the LEADER and owns everything that is shared - PCM staging, the frontend's
 * launches, the dense frames-major head input, the stream batch with its PCM and log-mel rings, the recording pool; the other members
 * are FOLLOWERS: they run only their head plan, on the leader's head input, launch no frontend and hold no PCM (their workspaces are
 * sized as nww_forward_features_dev sizes them).  A call runs exactly the frontend work the leader alone would run - one launch per
 * batch or pass, the leader's pool / edge / assembly launches on a recording's shared route, its whole / primed launches in a pool
 * call - then the k head plans, all on `stream` in member order.  DESIGN.md 4.8f.
 * Outputs are member-major [k][n]: member j's value for item i at j * n + i, n being B, nW or the number of listed streams; either
 * may be NULL.  Member j's logits and probabilities are bit-identical to the single-handle call on member j alone with the same input
 * - nww_forward_pcm; nww_forward_recording with the same max_batch; nww_stream_push_some on a batch of its own that received the same
 * push / reset calls (a listed stream that holds no window reads 0 / 0 for every member) - and do not depend on which member leads.
 * k = 1 is the plain call on members[0].  Profiling works per member; a follower's entry 0 (frontend) records nothing in a bank call.
 * Rules, checked before anything is launched or any ring is touched - a failing call writes no output and leaves every
 * nww_stream_filled_of as it was; the text names the offending member by its index:
 *   members non-NULL and k >= 1; every member non-NULL, finalized, distinct, on one device              NWW_ERR_INVALID
 *   no raw-PCM head (e2e_quartznet, e2e_cnn) among k > 1 members: a learned frontend shares nothing     NWW_ERR_INVALID
 *   identical frontends: sample_rate, n_fft, win_length, hop_length, n_mels, center, f_min, f_max, amin, db_multiplier equal, the
 *   window and mel filterbank tables byte-equal, loaded (frontend.window / frontend.mel_fb) or built in;
 *   the text names the first differing field                                                           NWW_ERR_INVALID
 *   every member consumes frames-major log-mel (an e2e_dnn planned in the reference's orientation, for
 *   instance under conv_arith = f32, does not)                                                         NWW_ERR_UNSUPPORTED
 *   the clip or window gives every member its own (in_rows, in_cols)                                   NWW_ERR_SHAPE
 *   the stream call: the leader has an open batch (NWW_ERR_STATE), idx as in nww_stream_push_some      NWW_ERR_INVALID
 * Errors go to nww_last_error(members[0]) (to nww_last_error(NULL) where there is no members[0]).  The dense [2][k][n] outputs of the
 * host-pointer variants live on the leader's handle, grow on demand and are freed by nww_destroy.
 * Streams: only the leader has a stream batch; open, reset, close, nww_stream_reset_some, nww_stream_filled_of and
 * nww_stream_pool_stats are the leader's existing calls.  The bank's stream entry point is the pool call, on a batch in any state; a
 * call that lists every stream of an aligned batch keeps it aligned, and the lock-step nww_stream_push* on the leader alone runs
 * afterwards as before.  There is no lock-step bank call: that path may keep conv rows instead of a dense window (CRNN), which leaves
 * a follower nothing to read - clients that tick together list every stream.
 * (Declared `extern` like the blocks above: the pinned count of declarations that start a line with their return type stays 48.)      */
/* the rules alone, for clips or windows of `window` samples: 0 or the error code                                                     */
extern int nww_bank_check(nww_handle* const* members, int32_t k, int32_t window);
/* d_pcm [B][N] -> d_logits / d_probs [k][B]; asynchronous on `stream` (NULL: the leader's own)                                        */
extern int nww_bank_forward_pcm_dev(nww_handle* const* members, int32_t k, const int16_t* d_pcm, int32_t B, int32_t N,
                                    float* d_logits, float* d_probs, void* stream);
/* host pointers; the clips are uploaded once, into the leader's staging; synchronises before it returns                               */
extern int nww_bank_forward_pcm(nww_handle* const* members, int32_t k, const int16_t* pcm, int32_t B, int32_t N, float* logits, float* probs);
/* every window of a recording (the rules of nww_forward_recording*, the route the leader plans): d_logits / d_probs [k][nW]          */
extern int nww_bank_forward_recording_dev(nww_handle* const* members, int32_t k, const int16_t* d_pcm, int32_t n_samples, int32_t window, int32_t hop,
                                          int32_t max_batch, float* d_logits, float* d_probs, void* stream);
/* host pointers; the recording is uploaded once.  n_windows_out may be NULL.                                                          */
extern int nww_bank_forward_recording(nww_handle* const* members, int32_t k, const int16_t* pcm, int32_t n_samples, int32_t window, int32_t hop,
                                      int32_t max_batch, float* logits, float* probs, int32_t* n_windows_out);
/* the listed streams of the leader's batch (idx, n and the chunk as in nww_stream_push_some): outputs [k][n], in idx order             */
extern int nww_bank_stream_push_some_dev(nww_handle* const* members, int32_t k, const int32_t* idx, int32_t n, const int16_t* d_chunk,
                                         float* d_logits, float* d_probs, void* stream);
extern int nww_bank_stream_push_some(nww_handle* const* members, int32_t k, const int32_t* idx, int32_t n, const int16_t* chunk,
                                     float* logits, float* probs);

/* ---- clips mixed on the device: SNR mixing and level scaling (augment_clips.py:45-79,201-231,246-259) --------------------------------
 * An ARENA is one int16 device buffer of arena_samples samples in which foregrounds and backgrounds lie back to back (2-byte alignment
 * only).  A call takes a HOST table of B items and writes int16 out[B][N]; the table goes up through slots of the handle's own pinned
 * and device buffers (an event per slot), the device gathers, measures and mixes.  What the reference draws at random - background,
 * crop, position, SNR, gain, level - the host decides and writes into the item; the arithmetic is fixed so that it is the same bits on
 * the host (csrc/mix_plan.h, tests/mix_oracle.py) and on the device.  With f[j] = fg[j] / 32768, b[i] = bg[(bg_start + i) % bg_len] / 32768:
 *   Sf = sum fg[j]^2, Sb = sum of the background's squares under the foreground (at start + j), P = max |background| over the N
 *   samples: exact integers.  The background is REAL iff bg_len > 0 and P >= 4 (the reference's peak > 1e-4).
 *   real:      scale in float64 from Sf, Sb (eps = 2^-23, background floor 0.005, scaled-foreground floor 0.01: _mix_snr), rounded
 *              to float32 once = s;  x[i] = b[i], and x[i] = b[i] + f[i - start] * s for start <= i < start + fg_len
 *   not real:  x[i] = f[i] for i < fg_len, 0 elsewhere (`start` is ignored)
 *   y = x * gain;  flags bit 0 (peak-normalise): pk = max |y| (1 if < 1e-8), z = y * (level / pk);  clear: z = y * level
 *   out[i] = (int16) trunc(clamp(z, -1, 1) * 32767)
 * Every float32 product and sum is rounded on its own (nothing contracted).  A clip depends on its own item alone: the same bits at
 * any B, at any position in the table.  DESIGN.md 4.8g.
 * Rules, checked on the host for EVERY item before anything is enqueued - a failing call launches nothing, takes no table slot and
 * returns NWW_ERR_INVALID with the item's index and the field's name in nww_last_error:
 *   1 <= fg_len <= N;  [fg_off, fg_off + fg_len) inside the arena;  bg_len >= 0, and for bg_len > 0 [bg_off, bg_off + bg_len)
 *   inside the arena and 0 <= bg_start < bg_len (bg_off and bg_start are not read when bg_len == 0);  0 <= start <= N - fg_len;
 *   snr_linear, gain and level finite and > 0;  no flag bit but bit 0.
 * N >= 1.  B == 0 returns NWW_OK and does nothing.  The handle must be finalized.
 * (Declared `extern` like the blocks above.)                                                                                        */
typedef struct nww_mix_item {
    int64_t fg_off, bg_off;            /* first sample of the foreground / background in the arena                       */
    int32_t fg_len, bg_len;            /* samples; bg_len == 0: no background                                            */
    int32_t bg_start;                  /* clip sample i reads background sample (bg_start + i) % bg_len                  */
    int32_t start;                     /* clip sample the foreground's first sample is mixed into                        */
    float snr_linear, gain, level;     /* 10^(snr_db / 20), 10^(gain_db / 20), target peak (bit 0 set) or volume factor */
    uint32_t flags;                    /* NWW_MIX_PEAK_NORMALISE; 48 bytes, no implicit padding                          */
} nww_mix_item;
#define NWW_MIX_PEAK_NORMALISE 1u
/* d_arena [arena_samples], items [B] (host) -> d_out [B][N]; asynchronous on `stream` (NULL: the handle's own); `items` may be reused
   as soon as the call returns                                                                                                        */
extern int nww_mix_dev(nww_handle* h, const int16_t* d_arena, int64_t arena_samples, const nww_mix_item* items, int32_t B, int32_t N,
                       int16_t* d_out, void* stream);
/* host pointers: the arena is uploaded, the clips are mixed and downloaded; synchronises before it returns                         */
extern int nww_mix(nww_handle* h, const int16_t* arena, int64_t arena_samples, const nww_mix_item* items, int32_t B, int32_t N, int16_t* out);
/* the clips mixed into the handle's PCM staging, then nww_forward_pcm_dev's path on them: d_logits / d_probs [B] (d_probs may be
   NULL), bit-identical to nww_forward_pcm on the output of nww_mix                                                                  */
extern int nww_mix_forward_pcm_dev(nww_handle* h, const int16_t* d_arena, int64_t arena_samples, const nww_mix_item* items, int32_t B, int32_t N,
                                   float* d_logits, float* d_probs, void* stream);
/* ... then nww_frontend_dev's path on them: d_logmel as nww_frontend_dev writes it                                                  */
extern int nww_mix_frontend_dev(nww_handle* h, const int16_t* d_arena, int64_t arena_samples, const nww_mix_item* items, int32_t B, int32_t N,
                                float* d_logmel, int32_t frames_major, void* stream);

/* ---- ... through a room impulse response (the reference's ApplyImpulseResponse, augment_clips.py:150-157) ----------------------------
 * With y[i] the float32 clip above (after the gain, before the level) and h[0 .. L) a float32 impulse response:
 *   w[i] = sum over k <= i, k < L of h[k] * y[i - k],  0 <= i < N        (convolve(mode = "full")[..., :N])
 * and the tail runs on w: pk = max |w| under bit 0 (1 if < 1e-8), z = w * ratio, out as above.  Taps at k >= N never reach the first N
 * outputs and are dropped.  The response's own scale is the caller's business (under bit 0 it cancels in level / pk).
 * The convolution is a float32 FFT of M real points per clip held in LDS (csrc/rir.hip): M is the smallest of 2048,
 * 8192 and 32768 with N + min(L_max, N) - 1 <= M - nww_rir_fft_size returns it, or 0 where none fits (every N <= 16384 fits with any
 * response).  The arithmetic is fixed (csrc/rir_plan.h, restated in tests/rir_oracle.py): the same bits on the host and the device, at
 * any B and any position in the table.  An item without a response (ir_id == -1) is the clip nww_mix gives, bit for bit.
 * Response SPECTRA are prepared once: nww_rir_prepare_dev takes K responses lying back to back in a float32 device buffer
 * (ir_off / ir_len: HOST arrays, samples) and writes float [K][M] (8-byte aligned) in the kernel's own order - opaque to callers, valid
 * for this N and M only.  A response with N + min(ir_len, N) - 1 > 32768 is NWW_ERR_INVALID with its index ("overlap-save not built"
 * into this route; pass NWW_RIR_SEGMENTED), and so are ir_len < 1, one that does not fit M, and an M that is none of the three; nothing
 * is truncated silently.  The call synchronises `stream` before it returns.
 * M = NWW_RIR_SEGMENTED selects the second route, for clips and responses of ANY length (N >= 1, ir_len >= 1): uniformly partitioned
 * overlap-save on the 32768-point transform.  The first min(ir_len, N) taps are cut into nww_rir_parts(N, ir_len) partitions of 16384
 * taps, the clip into segments of 16384 outputs; a segment is the float32 sum, partition after partition, of its windows' transforms
 * (csrc/rir_plan.h, restated in tests/rir_seg_oracle.py: again the same bits on the host and the device, at any B), and the peak is
 * taken over the whole clip before the tail.  d_spectra then holds nww_rir_spectra_floats(K, N, max ir_len, NWW_RIR_SEGMENTED) floats
 * (16-byte aligned; it carries every response's partition count) and is valid for this N, and for n_irs <= K, only; the mixing calls
 * keep 4 B N + 4 B ceil(N / 16384) bytes of float32 scratch on the handle.  Every other rule and message is the same on both routes.
 * The mixing calls take a second HOST table rir_items [B] next to `items` (NULL: no response anywhere, M / d_spectra / n_irs are not
 * read and the call is nww_mix_*'s); both tables go up in ONE copy through the same slot.  Checked on the host for every item before
 * anything is enqueued, after the rules above: ir_id in [-1, n_irs), reserved == 0, and M one of the three sizes with N <= M (the M the
 * spectra were prepared at) - NWW_ERR_INVALID names the index and the field, nothing is launched and no slot is taken.                */
typedef struct nww_rir_item { int32_t ir_id; uint32_t reserved; } nww_rir_item;   /* -1: none; reserved == 0 */
extern int32_t nww_rir_fft_size(int32_t N, int32_t max_ir_len);
#define NWW_RIR_SEGMENTED (-1)         /* as M: the segmented route */
/* partitions of a response of max_ir_len taps against clips of N; 0 for arguments below 1                                           */
extern int32_t nww_rir_parts(int32_t N, int32_t max_ir_len);
/* floats of d_spectra for K responses at M (a transform size: K * M; NWW_RIR_SEGMENTED: see above); 0 for bad arguments             */
extern int64_t nww_rir_spectra_floats(int32_t K, int32_t N, int32_t max_ir_len, int32_t M);
extern int nww_rir_prepare_dev(nww_handle* h, const float* d_irs, const int64_t* ir_off, const int32_t* ir_len, int32_t K, int32_t N, int32_t M,
                               float* d_spectra, void* stream);
extern int nww_mix_rir_dev(nww_handle* h, const int16_t* d_arena, int64_t arena_samples, const float* d_spectra, int32_t n_irs, int32_t M,
                           const nww_mix_item* items, const nww_rir_item* rir_items, int32_t B, int32_t N, int16_t* d_out, void* stream);
/* arena and out are host pointers as in nww_mix; d_spectra stays a device pointer (nww_rir_prepare_dev wrote it)                     */
extern int nww_mix_rir(nww_handle* h, const int16_t* arena, int64_t arena_samples, const float* d_spectra, int32_t n_irs, int32_t M,
                       const nww_mix_item* items, const nww_rir_item* rir_items, int32_t B, int32_t N, int16_t* out);
extern int nww_mix_rir_forward_pcm_dev(nww_handle* h, const int16_t* d_arena, int64_t arena_samples, const float* d_spectra, int32_t n_irs, int32_t M,
                                       const nww_mix_item* items, const nww_rir_item* rir_items, int32_t B, int32_t N, float* d_logits,
                                       float* d_probs, void* stream);
extern int nww_mix_rir_frontend_dev(nww_handle* h, const int16_t* d_arena, int64_t arena_samples, const float* d_spectra, int32_t n_irs, int32_t M,
                                    const nww_mix_item* items, const nww_rir_item* rir_items, int32_t B, int32_t N, float* d_logmel,
                                    int32_t frames_major, void* stream);

/* ---- pitch shift between the gain and the response (csrc/pitch.hip, csrc/pitch_plan.h) -------------------------
 * The reference applies PitchShift(+-2 semitones, p = 0.5) between Gain and ApplyImpulseResponse (augment_clips.py:150-157).  What is
 * restated is a DEFINITION of that construction, not the library's samples: a time stretch by a phase vocoder without phase scaling,
 * then a windowed-sinc resampler back to N samples, at a rational ratio r = p / q (r > 1 raises the pitch):
 *   STFT       n_fft 512, hop 128, periodic Hann, centred with reflect padding: T = 1 + N / 128 frames of 257 bins (N > 256)
 *   vocoder    T_out = ceil(T p / q) frames; frame t reads X[i], X[i + 1] at i = (t q) div p, alpha = ((t q) mod p) / p (frames >= T are
 *              zero); magnitude alpha |X1| + (1 - alpha) |X0|; phase of frame 0 that of X[0], then advanced by angle(X1) - angle(X0)
 *   ISTFT      overlap-add over the summed squared window, centre trimmed: S = 128 (T_out - 1) samples
 *   resample   y[n] = sum_k s[k] g(n p / q - k), n < ceil(S q / p), g a Hann-windowed sinc of six zero crossings a side at rolloff
 *              0.99 (cutoff 0.99 min(1, q / p)); cropped or zero-padded to N
 * The transform length, hop and window are this project's own.  y takes the place of the mixed clip after the gain in everything
 * behind it: the response, the peak, the level and the int16 tail.  The float32 arithmetic is fixed in csrc/pitch_plan.h (restated in
 * tests/pitch_oracle.py): the same bits on the host and the device, at any B and any place in the table.
 * nww_pitch_set_ratios validates K <= 64 ratios (1 <= num, den <= 256, 2^(-4/12) <= num / den <= 2^(4/12)), builds their resampler
 * tables on the host and uploads them onto the handle (it waits for the device); K = 0 clears them.
 * The nww_mix_aug_* calls are the nww_mix_rir_* calls plus a third HOST table pitch_items [B] (NULL: the nww_mix_rir_* call; rir_items
 * NULL as well: nww_mix_*'s); a clip with pitch_id == -1 comes out bit-identical to the same clip without the table.  Checked on the
 * host before anything is enqueued, after the rules above: ratios set, 256 < N <= 2^28, pitch_id in [-1, K), reserved == 0 -
 * NWW_ERR_INVALID names the index and the field, nothing is launched, no slot is taken and the ratios stay what they were.  The calls
 * keep 4 (N + 128 ceil(T 162 / 128)) bytes of float32 scratch per shifted clip on the handle (about 9.1 N), grown on demand; calls on
 * one handle share it, so they go on one stream or are ordered by the caller.                                                         */
typedef struct nww_pitch_item { int32_t pitch_id; uint32_t reserved; } nww_pitch_item;   /* -1: none; reserved == 0 */
extern int nww_pitch_set_ratios(nww_handle* h, const int32_t* num, const int32_t* den, int32_t K);
extern int nww_mix_aug_dev(nww_handle* h, const int16_t* d_arena, int64_t arena_samples, const float* d_spectra, int32_t n_irs, int32_t M,
                           const nww_mix_item* items, const nww_rir_item* rir_items, const nww_pitch_item* pitch_items, int32_t B, int32_t N,
                           int16_t* d_out, void* stream);
extern int nww_mix_aug(nww_handle* h, const int16_t* arena, int64_t arena_samples, const float* d_spectra, int32_t n_irs, int32_t M,
                       const nww_mix_item* items, const nww_rir_item* rir_items, const nww_pitch_item* pitch_items, int32_t B, int32_t N,
                       int16_t* out);
extern int nww_mix_aug_forward_pcm_dev(nww_handle* h, const int16_t* d_arena, int64_t arena_samples, const float* d_spectra, int32_t n_irs,
                                       int32_t M, const nww_mix_item* items, const nww_rir_item* rir_items, const nww_pitch_item* pitch_items,
                                       int32_t B, int32_t N, float* d_logits, float* d_probs, void* stream);
extern int nww_mix_aug_frontend_dev(nww_handle* h, const int16_t* d_arena, int64_t arena_samples, const float* d_spectra, int32_t n_irs,
                                    int32_t M, const nww_mix_item* items, const nww_rir_item* rir_items, const nww_pitch_item* pitch_items,
                                    int32_t B, int32_t N, float* d_logmel, int32_t frames_major, void* stream);

/* ---- recordings at their own sample rate brought to the target rate (csrc/resample.hip, csrc/resample_plan.h) ------
 * The reference resamples and downmixes on every path into 16 kHz mono: torchaudio.transforms.Resample(clip_sr, 16000), then the mean
 * over the channels (augment_clips.py:31-43, transform_clips.py:65-93, utils/audio_preprocess.py:55-90).  What is restated is a
 * DEFINITION of that resampler's construction - sinc_interp_hann, lowpass_filter_width 6, rolloff 0.99 - not the library's samples.
 * A recording has L frames of C interleaved channels at rate fs; the target rate is ft; g = gcd(fs, ft), p = fs / g, q = ft / g
 * (p / q > 1 lowers the rate).
 *   downmix    m[k] = (0.0f + c_0[k] + .. + c_{C-1}[k]) / (float)C: channels in ascending order, one correctly rounded division; C = 1
 *              is the sample itself.  The reference takes the mean after resampling: equal in exact arithmetic (both are linear).
 *   resample   M = ceil(L q / p) outputs; output n sits at input position n p / q:
 *              v[n] = 0.0f + sum over ascending j of m[k0 + j] g[phase][j],  phase = n mod q,  k0 = (n div q) p + (phase p) div q + j0,
 *              taps with k0 + j outside [0, L) left out; every product and sum rounded on its own
 *   taps       g[phase][j] = c sinc(c x) cos^2(pi c x / 12) where |c x| < 6 and an exact 0 elsewhere, x = frac - (j0 + j),
 *              frac = ((phase p) mod q) / q, c = 0.99 min(1, q / p); float64, rounded once.  j0 = 1 - ceil(6 / c), 2 ceil(6 / c) taps a
 *              phase (ceil(6 / c) in integers: ceil(200 p / (33 q)) where p > q, 7 otherwise): 38 at 3/1, 34 at 441/160, 18 at 441/320
 *   formats    source NWW_PCM_S16 (the float of its value) or NWW_PCM_F32 (as given; a non-finite sample is the caller's business).
 *              Destination F32: v 2^-15 from an S16 source (exact), v from an F32 source - the units torchaudio.load gives.
 *              Destination S16: (int16) rint(clamp(u, -32768, 32767)), nearest even, u = v from an S16 source and v 32768 from an F32
 *              source: a full-scale square wave overshoots to 37 708 at 48 k -> 16 k and comes out as 32 767, never wrapped
 *   rate_id -1 the recording is already at the target rate: downmixed and converted only (the reference's `if clip_sr != sr`), no filter
 * The float32 arithmetic is fixed in csrc/resample_plan.h (restated in tests/resample_oracle.py): the same bits on the host and the
 * device, at any B and any place in the table.
 * The ratios a table's rate_id names are set once on the handle: terms in [1, 1024], 1/4 <= num / den <= 12, K <= 16 (K = 0 clears
 * them); the tables are built on the host and uploaded, the call waits for the device.  They are separate from the pitch ratios.
 * A call takes a HOST table of B items (reusable once it returns) through a slot of the handle, as the mixing calls do.  Rules, checked
 * on the host for EVERY item before anything is enqueued - a failing call launches nothing, takes no slot, leaves the ratios alone and
 * returns NWW_ERR_INVALID with the item's index and the field's name in nww_last_error:
 *   ratios set unless every rate_id is -1;  1 <= src_frames <= 2^30;  1 <= channels <= 8;  [src_off, src_off + src_frames channels)
 *   inside src_values;  rate_id in [-1, K);  reserved == 0;  both formats known;  [dst_off, dst_off + len) inside dst_values, len the
 *   item's outputs;  destination ranges ascending and disjoint across the table (dst_off[i] >= dst_off[i - 1] + len[i - 1]): no two
 *   workgroups write one sample.
 * B == 0 returns NWW_OK and does nothing.  The handle must be finalized.                                                             */
#define NWW_PCM_S16 0
#define NWW_PCM_F32 1
typedef struct nww_resample_item {
    int64_t src_off;                   /* first value of the recording in the source buffer (values, not frames)          */
    int64_t dst_off;                   /* first output in the destination buffer                                         */
    int32_t src_frames;                /* L                                                                              */
    int32_t channels;                  /* C, interleaved                                                                 */
    int32_t rate_id;                   /* the ratio, or -1: already at the target rate                                   */
    uint32_t reserved;                 /* 0; 32 bytes, no implicit padding                                               */
} nww_resample_item;
extern int nww_resample_set_ratios(nww_handle* h, const int32_t* num, const int32_t* den, int32_t K);
/* ceil(frames den / num); 0 for bad arguments (frames outside [1, 2^30], a ratio out of range)                                       */
extern int64_t nww_resample_length(int64_t frames, int32_t num, int32_t den);
/* d_src [src_values] of src_format, items [B] (host) -> d_dst [dst_values] of dst_format; asynchronous on `stream` (NULL: the
   handle's own)                                                                                                                      */
extern int nww_resample_dev(nww_handle* h, const void* d_src, int64_t src_values, int32_t src_format, const nww_resample_item* items, int32_t B,
                            void* d_dst, int64_t dst_values, int32_t dst_format, void* stream);
/* host pointers: the source is uploaded, the items' destination ranges are downloaded (what lies between them is left alone);
   synchronises before it returns                                                                                                     */
extern int nww_resample(nww_handle* h, const void* src, int64_t src_values, int32_t src_format, const nww_resample_item* items, int32_t B,
                        void* dst, int64_t dst_values, int32_t dst_format);

/* ---- embedding-mode preprocessor state on the device (S lock-step streams) -------------------------------
 * Replaces the buffers and windowing of nanowakeword/data/AudioFeatures.py around its two ONNX models
 * (melspectrogram.onnx / embedding_model.onnx: un-vendored release binaries, pluggable here - the caller runs
 * them and hands their outputs over, host or device pointers):
 *   melspectrogram_buffer (np.ones((76,32)) at reset, newest 970 frames kept)      AudioFeatures.py:107,119,393-398
 *   melspec_transform x/10 + 2 (raw = 1)                                            :124,146
 *   76-frame windows every 8 frames, one per new 80 ms chunk, oldest first          :434-440
 *   feature_buffer (newest 120 rows) and get_features(n) = its last n rows          :446-457
 *   batch path: -80 padding to the longest clip, all windows of a clip              :188-227, 231-295
 * The handle must be a finalized feature-mode head with in_cols == emb_dim; nww_emb_forward scores every
 * stream on get_features(in_rows) without the features leaving the device.                                    */
int nww_emb_open(nww_handle* h, int32_t n_streams, int32_t mel_bins, int32_t emb_dim, int32_t mel_cap, int32_t feat_cap);
int nww_emb_reset(nww_handle* h);              /* mel ring = ones(76, bins), feature ring empty (re-seed it with nww_emb_push_features) */
int nww_emb_close(nww_handle* h);
int nww_emb_state(const nww_handle* h, int32_t* mel_frames, int32_t* feature_rows);
/* mel [n_streams][n_frames][mel_bins] float32: the mel model's output for the newest audio of every stream      */
int nww_emb_push_mel(nww_handle* h, const float* mel, int32_t n_frames, int32_t on_device, int32_t raw);
/* windows [n_streams][n_valid][76][mel_bins]: the windows of the n_chunks newest 80 ms chunks, oldest first       */
int nww_emb_windows(nww_handle* h, int32_t n_chunks, float* windows, int32_t on_device, int32_t* n_valid);
/* emb [n_streams][k][emb_dim]: the embedding model's rows for those windows                                       */
int nww_emb_push_features(nww_handle* h, const float* emb, int32_t k, int32_t on_device);
/* out [n_streams][n_out][emb_dim], n_out = min(n_frames, rows held)                                               */
int nww_emb_get_features(nww_handle* h, int32_t n_frames, float* out, int32_t on_device, int32_t* n_out);
/* logits / probs [n_streams] (host pointers, either may be NULL)                                                 */
int nww_emb_forward(nww_handle* h, float* logits, float* probs);
/* batch path. mel [B][F][bins] -> windows [B][n_windows][76][bins], n_windows = (F - 76) / 8 + 1                 */
int nww_emb_window_batch(nww_handle* h, const float* mel, int32_t B, int32_t F, int32_t bins, float* windows,
                         int32_t on_device, int32_t* n_windows);
/* packed: B ragged spectrograms back to back ([sum(frames)][bins], host) -> out [B][Fmax][bins] (host)           */
int nww_emb_pad_batch(nww_handle* h, const float* packed, const int32_t* frames, int32_t B, int32_t bins, int32_t Fmax,
                      float pad, int32_t raw, float* out);

/* ---- multi-GPU: batch split, one RCCL all-gather of the per-clip logits ------------------------
 * One process (and one handle) per GPU; every rank scores its own contiguous shard of the clips.  The path's only
 * exchange is an all-gather of 4 bytes per clip over RCCL / xGMI, enqueued on the same stream as the kernels.
 * The reference has no counterpart (it is single-process).  RCCL is bound at run time, so single-GPU users never
 * load it.  Rank 0 creates the 128-byte id and hands it to the other ranks by any means (file, socket, MPI,
 * torch.distributed - bench.py broadcasts it); then every rank calls nww_comm_init.                            */
#define NWW_COMM_ID_BYTES 128
int nww_comm_unique_id(void* id128);
int nww_comm_init(nww_handle* h, int32_t rank, int32_t world, const void* id128);
int nww_comm_destroy(nww_handle* h);
/* d_send [count] -> d_recv [world][count] on every rank; asynchronous on `stream`                                */
int nww_all_gather_logits(nww_handle* h, const float* d_send, float* d_recv, int32_t count, void* stream);
/* forward of this rank's B clips + all-gather into d_all_logits [world][B], one stream, no host hop               */
int nww_forward_pcm_gather_dev(nww_handle* h, const int16_t* d_pcm, int32_t B, int32_t N, float* d_all_logits, void* stream);
/* the same step with the all-gather on the handle's OWN stream behind an event: step k + 1's kernels (on `stream`) never wait for
   step k's RCCL latency.  Alternate two d_all_logits buffers; call k waits (device-side) for gather k - 2 before it reuses them.
   nww_gather_fence makes `stream` wait for every gather issued so far - after it the gathered vectors are valid in stream order.
   nww_gather_overlap_ms (host-synchronising, tests / tools): ms from the latest step's start to the end of the previous step's gather */
int nww_forward_pcm_gather_async_dev(nww_handle* h, const int16_t* d_pcm, int32_t B, int32_t N, float* d_all_logits, void* stream);
int nww_gather_fence(nww_handle* h, void* stream);
int nww_gather_overlap_ms(nww_handle* h, float* ms);

const char* nww_version(void);

#ifdef __cplusplus
}
#endif
#endif /* NWW_H */
