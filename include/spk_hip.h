/*
 * spk_hip.h — C ABI of libspk_hip.so, the MI355X (gfx950) speaker-embedding hot path.
 *
 * Plain C, POD arguments only: device pointers are raw `float*`/`int64_t*` (owned by the
 * caller, e.g. the torch caching allocator), streams are `hipStream_t` passed as `void*`.
 * Every entry point returns 0 on success or a negative SPK_E_* code; the message of the
 * last failure on the calling thread is available from spk_last_error().  No C++
 * exception crosses this boundary.  Handles are immutable after creation, so one handle
 * may be used from several streams concurrently, each forward with its own workspace (all
 * per-forward state, the fp16x3 range word included, lives in the workspace); forward()
 * allocates nothing (the caller provides a workspace sized by spk_model_workspace_bytes())
 * and never synchronises the host, so it can be captured into a hipGraph.
 *
 * Which reference interface each entry point replaces (paths relative to the reference
 * repo nanless/3D-Speaker):
 *   spk_fbank_f32        speakerlab/process/processor.py:133-158 (FBank.__call__ ->
 *                        torchaudio.compliance.kaldi.fbank) and the C++ runtime's
 *                        FbankComputer::compute_feature runtime/onnxruntime/feature/feature_fbank.cpp:22-91
 *   spk_resample_f32     torchaudio.functional.resample as called by load_audio,
 *                        speakerlab/utils/fileio.py:105-129
 *   spk_vad_energy_f32, spk_vad_apply_intervals_f32
 *                        the per-sample numpy of speakerlab/bin/infer_diarization.py's VAD front:
 *                        the frame energies (:403-413 and the VAD's own) and the masked copy (:560-601)
 *   spk_model_create     model construction + strict load_state_dict in
 *                        speakerlab/bin/infer_sv_batch.py:247-253 (and the ONNX session
 *                        runtime/onnxruntime/model/speaker_embedding_model.cpp:7-40)
 *   spk_model_forward    nn.Module.forward of ERes2NetV2.py:235-254, ERes2Net.py:208-231,
 *                        ECAPA_TDNN.py:430-463, DTDNN.py:111-115 (and
 *                        OnnxSpeakerEmbeddingModel::extract_embedding speaker_embedding_model.cpp:42-69)
 *   spk_cosine_affinity  sklearn cosine_similarity as used by speakerlab/process/cluster.py:59-62,150
 *                        and speakerlab/bin/compute_score_metrics.py:110-114
 *   spk_cosine_topk      the consumers of the row-block affinity: best matches
 *                        per row / threshold counts, the affinity never materialised
 *   spk_cosine_trials    the per-trial cosine_similarity loop of compute_score_metrics.py:102-118
 *   spk_ahc_average      AHCluster.__call__ after the affinity, speakerlab/process/cluster.py:139-156
 *                        (fastcluster linkage(method='average') + fcluster(criterion='distance'))
 *   spk_ahc_average_batched  the same step for several recordings in one launch
 *   spk_topk_stats, spk_cosine_cohort_stats, spk_cosine_trials_norm
 *                        nothing in the reference: the numpy partition / mean / std of cohort
 *                        scores (S-norm / AS-norm) users write next to compute_score_metrics.py
 *   spk_pair_cosine_stats    the pair loop of speakerlab/bin/check_single_speaker.py
 *                        (check_single_speaker: cosine of every segment pair, min and mean)
 */
#ifndef SPK_HIP_H
#define SPK_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SPK_OK 0
#define SPK_E_INVALID (-1)     /* bad argument / shape */
#define SPK_E_HIP (-2)         /* HIP runtime error */
#define SPK_E_WEIGHTS (-3)     /* missing or mis-shaped state_dict tensor */
#define SPK_E_DEVICE (-4)      /* handle used on another device */
#define SPK_E_WORKSPACE (-5)   /* workspace too small */
#define SPK_E_UNSUPPORTED (-6)

/* architectures (the four models on the north-star path) */
#define SPK_ARCH_ERES2NETV2 1  /* speakerlab.models.eres2net.ERes2NetV2.ERes2NetV2 */
#define SPK_ARCH_ERES2NET 2    /* speakerlab.models.eres2net.ERes2Net.ERes2Net     */
#define SPK_ARCH_ECAPA 3       /* speakerlab.models.ecapa_tdnn.ECAPA_TDNN.ECAPA_TDNN */
#define SPK_ARCH_CAMPPLUS 4    /* speakerlab.models.campplus.DTDNN.CAMPPlus         */
#define SPK_ARCH_RESNET 5      /* speakerlab.models.resnet.ResNet.ResNet (BasicBlock, TSTP) */
#define SPK_ARCH_RES2NET 6     /* speakerlab.models.res2net.Res2Net.Res2Net (TSTP)  */

typedef struct spk_model spk_model_t;

/* One state_dict tensor, HOST memory, float32 contiguous (int tensors such as
 * num_batches_tracked may be passed with data == NULL).  Keys are the reference's. */
typedef struct {
  const char* name;
  const float* data;
  int32_t ndim;
  int64_t shape[4];
} spk_weight_t;

/* Constructor arguments of the reference module (only those that shape the graph). */
#define SPK_PRECISION_FP32 0
#define SPK_PRECISION_FP16 1
#define SPK_POOL_TSTP 0
#define SPK_POOL_TAP 1
#define SPK_POOL_TSDP 2
#define SPK_POOL_ASTP 3

typedef struct {
  int32_t arch;
  int32_t feat_dim;       /* 80 */
  int32_t embed_dim;      /* embedding_size / lin_neurons */
  int32_t m_channels;     /* ERes2Net*: m_channels */
  int32_t base_width;     /* ERes2NetV2: baseWidth (26); ERes2Net: 32 */
  int32_t scale;          /* ERes2Net*: scale (2) */
  int32_t expansion;      /* ERes2Net*: expansion (2) */
  int32_t two_emb_layer;  /* ERes2Net*: two_emb_layer */
  int32_t channels[5];    /* ECAPA: channels */
  int32_t kernel_sizes[5];/* ECAPA: kernel_sizes */
  int32_t dilations[5];   /* ECAPA: dilations */
  int32_t precision;      /* SPK_PRECISION_FP32 (0, default): fp32-accurate (fp16x3 split
                             products); SPK_PRECISION_FP16 (1): one fp16 MFMA product per
                             multiply, fp32 accumulation -- BASELINE config C3's reduced-
                             precision mode (cosine >= 0.9999 to the reference) */
  int32_t pooling;        /* ERes2Net*: pooling_func -- SPK_POOL_TSTP (0, default), SPK_POOL_TAP (1),
                             SPK_POOL_TSDP (2), SPK_POOL_ASTP (3, global_context_att=False)
                             (pooling_layers.py:10-104) */
  int32_t reserved[6];
} spk_model_config_t;

/* ABI revision: 2 (spk_model_range_check's seven-argument form, spk_model_config_t.pooling), additive
 * level 1: spk_fbank_chunks_f32; level 2: spk_pair_cosine_sizes, spk_pair_cosine_stats,
 * spk_pair_cosine_plan; level 3: spk_cosine_sim_workspace_bytes, spk_cosine_rows_topk,
 * spk_cosine_triu_stats, spk_cosine_triu_hist; level 4: spk_cosine_verif_workspace_bytes,
 * spk_cosine_verif_moments, spk_cosine_verif_digits.  Entries are only ever added inside a revision, so spk_version()
 * still returns 2; a caller that needs an added entry looks its symbol up. */
int spk_version(void);
const char* spk_last_error(void);

/* Kaldi log-mel Fbank of a ragged batch.  wav: device float32 samples of all utterances
 * back to back; wav_offsets/frame_offsets: DEVICE int64 arrays of n_utt+1 entries (sample
 * and frame starts; frames = 1 + (len-400)/160).  feats: device [total_frames, n_mels]. */
int spk_fbank_f32(const float* wav, const int64_t* wav_offsets, int32_t n_utt, float* feats,
                  const int64_t* frame_offsets, int32_t n_mels, int32_t mean_nor, void* stream);

/* Same, written as a zero-padded batch [n_utt, t_max, n_mels]: utterance u at rows
 * [u * t_max, u * t_max + frames_u) (frames_u from frame_offsets), its remaining rows 0.
 * The input of spk_model_forward_lengths for variable-length batches. */
int spk_fbank_f32_padded(const float* wav, const int64_t* wav_offsets, int32_t n_utt, float* feats,
                         const int64_t* frame_offsets, int32_t t_max, int32_t n_mels, int32_t mean_nor, void* stream);

/* Fbank of circle-padded chunks of one device signal, without materialising them: the
 * circle_pad of the diarization pipeline's sub-segment extraction (speakerlab/bin/
 * infer_diarization.py do_emb_extraction) done in the kernel's own addressing.
 *   wav          device float32 [wav_len]: one recording, or several back to back;
 *   chunk_start, chunk_len  DEVICE int64 [n_chunks];
 *   sample i of chunk c, 0 <= i < pad_len, is wav[chunk_start[c] + i % chunk_len[c]];
 *   feats        device [n_chunks, T, n_mels], T = 1 + (pad_len - 400) / 160.
 * The rows have exactly the bits spk_fbank_f32 writes for the gathered [n_chunks, pad_len] batch
 * (same kernel, same arithmetic in the same order; only the sample addresses differ).
 * Enqueues only.  The two arrays are not read on the host, so their contract is the caller's:
 * every chunk must satisfy chunk_len >= 1, chunk_start >= 0 and chunk_start + chunk_len <= wav_len;
 * anything else reads outside the signal.  (speakerlab._hip.fbank_chunks checks it on its host
 * copies before the upload.)  SPK_E_INVALID: n_chunks < 0, pad_len < 400 or above 2^31 - 1,
 * wav_len < 1, n_mels outside [4, 128] or one the mel tables cannot be built for, a null pointer
 * with n_chunks > 0.  n_chunks == 0: SPK_OK, nothing is launched.  SPK_E_UNSUPPORTED: a host-only
 * build of the library without kernels. */
int spk_fbank_chunks_f32(const float* wav, int64_t wav_len, const int64_t* chunk_start, const int64_t* chunk_len,
                         int32_t n_chunks, int64_t pad_len, float* feats, int32_t n_mels, int32_t mean_nor,
                         void* stream);

/* Sample-rate conversion in front of the Fbank: torchaudio.functional.resample with its defaults
 * (Hann-windowed sinc, lowpass_filter_width 6, rolloff 0.99), the resampler behind the reference's
 * load_audio (speakerlab/utils/fileio.py:105-129).  Rates are reduced by their gcd to o (orig) and
 * n (new); every tap of the polyphase table is computed in double and rounded once to fp32; every
 * output is one fp32 FMA chain in ascending tap order, so an utterance's result has the same bits
 * alone and inside any batch.  Error codes of all three: a non-positive rate SPK_E_INVALID; equal
 * rates SPK_E_INVALID from spk_resample_taps / spk_resample_f32 (nothing to resample;
 * spk_resample_out_len returns L); a table above 8 MiB (n_phases * n_taps * 4 bytes, e.g. 44101 ->
 * 16000) SPK_E_UNSUPPORTED from spk_resample_taps / spk_resample_f32. */
/* ceil(new*L/orig) in gcd-reduced rates (torchaudio.functional.resample's output length). */
int spk_resample_out_len(int64_t L, int32_t orig_freq, int32_t new_freq, int64_t* out_len);
/* Polyphase tap table the kernel uses (diagnostics, tests; host memory, no GPU needed):
 * n_phases = new/g, n_taps = 2*width + orig/g; taps (may be NULL to query sizes) [n_phases][n_taps]. */
int spk_resample_taps(int32_t orig_freq, int32_t new_freq, int32_t* n_phases, int32_t* n_taps,
                      int32_t* width, float* taps, size_t taps_len);
/* Ragged batch: wav / out device float32, offsets DEVICE int64 [n_utt+1]; out_offsets[u+1]-out_offsets[u]
 * must equal spk_resample_out_len of utterance u.  Enqueues only (the first call for a rate pair
 * on a device builds and uploads its table, synchronously; later calls reuse it).  Samples before
 * the first and past the last of an utterance read as zero; nothing outside the declared output
 * ranges is written; the output buffer has the layout spk_fbank_f32 reads. */
int spk_resample_f32(const float* wav, const int64_t* wav_offsets, int32_t n_utt, int32_t orig_freq,
                     int32_t new_freq, float* out, const int64_t* out_offsets, void* stream);

/* VAD front end of the diarization pipeline, 16 kHz only: the O(L) arithmetic in front of the
 * frame- and segment-level decisions, which stay on the host (speakerlab/utils/vad_post.py).
 *
 * spk_vad_energy_f32: one pass over a ragged batch (wav device float32, offsets DEVICE int64
 * [n_utt+1], the convention of spk_fbank_f32 / spk_resample_f32).  Every sample is first clipped
 * to [-1, 1]; per utterance of length L two mean-square tracks are written:
 *   e16 (device float64) [L / 256]: every non-overlapping 16 ms frame, the quantity under the
 *       energy VAD's 10 log10(. + 1e-12);
 *   e20 (device float32) [n20], n20 = (L - 320) / 160 + 1 for L >= 320, else 0: every 20 ms window
 *       at a 10 ms hop, the `en` of vad_post.frame_energy.
 * e16_offsets[u+1]-e16_offsets[u] and e20_offsets[u+1]-e20_offsets[u] must equal spk_vad_energy_sizes
 * of utterance u.  Squares and sums are fp64 in a fixed order counted from the utterance's own first
 * sample (quads of 4 samples, blocks of 32 = 8 quads, a hop = 5 blocks, a frame = 8 blocks, each
 * added in ascending order, no FMA contraction), e16 = frame / 256.0 and
 * e20[j] = float(hop[j] + hop[j+1]) / 320.0f, so an utterance has the same bits alone and inside any
 * batch.  Utterances shorter than a frame / a window write nothing to that track; nothing outside
 * the declared ranges is written.  Non-finite samples are outside the contract: np.clip propagates
 * a NaN, the kernel's fminf / fmaxf do not.  Enqueues only.
 *
 * spk_vad_apply_intervals_f32: out[i] = wav[i] for i inside one of the n_iv intervals
 * [starts[k], ends[k]) (DEVICE int64, sorted, disjoint, within [0, L]), else 0: the device form of
 * vad_post.apply_mask on the unclipped signal.  n_iv == 0 zeroes the output (starts / ends may then
 * be NULL); L == 0 launches nothing.  Enqueues only.
 *
 * Errors: n_utt < 0, L < 0, n_iv < 0 or a null pointer SPK_E_INVALID (spk_vad_energy_f32 with
 * n_utt == 0 succeeds and launches nothing); an e16 that is not 8-byte aligned SPK_E_INVALID; a
 * library built without the kernels SPK_E_UNSUPPORTED from the two launching entries.  Nothing is
 * written on an error. */
/* L / 256 and (L - 320) / 160 + 1 (0 below 320): host arithmetic, no GPU needed. */
int spk_vad_energy_sizes(int64_t L, int64_t* n16, int64_t* n20);
int spk_vad_energy_f32(const float* wav, const int64_t* wav_offsets, int32_t n_utt, double* e16,
                       const int64_t* e16_offsets, float* e20, const int64_t* e20_offsets, void* stream);
int spk_vad_apply_intervals_f32(const float* wav, int64_t L, const int64_t* starts, const int64_t* ends,
                                int64_t n_iv, float* out, void* stream);

/* Build a handle on the CURRENT HIP device: folds BatchNorm into conv weights, packs them
 * for the kernels and uploads them (synchronous, once per model). */
int spk_model_create(const spk_model_config_t* cfg, const spk_weight_t* weights, int32_t n_weights,
                     spk_model_t** out);
int spk_model_destroy(spk_model_t* model);

/* Workspace bytes needed by spk_model_forward for a [B, T, feat_dim] batch. */
int spk_model_workspace_bytes(spk_model_t* model, int32_t B, int32_t T, size_t* bytes);

/* feats: device [B, T, feat_dim] float32; emb_out: device [B, embed_dim] float32. */
int spk_model_forward(spk_model_t* model, const float* feats, int32_t B, int32_t T, void* workspace,
                      size_t workspace_bytes, float* emb_out, void* stream);

/* Variable-length batch: feats is [B, T, feat_dim] with utterance b occupying frames
 * [0, lengths[b]) (lengths: DEVICE int32 [B]).  lengths == NULL is spk_model_forward.
 *  - CAM++ (2 <= lengths[b] <= T): frames past lengths[b] are
 *    ignored, every embedding equals the forward of that utterance alone (no padding
 *    enters the computation).  Replaces running DTDNN.py:111-115 once per utterance.
 *  - ECAPA-TDNN (1 <= lengths[b] <= T): the reference's forward(x, lengths)
 *    (ECAPA_TDNN.py:209-287, 430-454): the convolutions run over the padded batch, the SE
 *    squeeze means and the attentive-pooling statistics cover frames [0, lengths[b]) only.
 *    (The reference takes RELATIVE lengths; the Python module converts them with the
 *    reference's own mask arithmetic, length_to_mask :11-27.)
 * Other architectures return SPK_E_UNSUPPORTED for a non-NULL lengths. */
int spk_model_workspace_bytes_lengths(spk_model_t* model, int32_t B, int32_t T, int32_t ragged, size_t* bytes);
int spk_model_forward_lengths(spk_model_t* model, const float* feats, int32_t B, int32_t T, const int32_t* lengths,
                              void* workspace, size_t workspace_bytes, float* emb_out, void* stream);

/* fp16x3 range guard, resolved on the device.  The default kernels represent every GEMM
 * operand as two fp16 values (fp32-accurate, csrc/conv_gemm.hip); a value at or past fp16's
 * range (65504) would saturate.  Every producer of an unbounded activation (and the input
 * check) raises a range word in the caller's workspace -- one per forward, zeroed when the
 * forward starts -- to the largest value it wrote once that reaches 2^14.  ECAPA-TDNN and
 * CAM++ GEMMs then split their operands scaled by a power of two taken from the word (exact,
 * no re-run); ERes2Net* / ResNet re-run the flagged plan segment on exact-fp32 MFMA kernels,
 * launched behind it on the same stream and gated on that word.  spk_model_forward* therefore
 * only enqueue (no host synchronisation), and concurrent forwards on different streams with
 * different workspaces never see each other's word.  spk_model_range_check() reports
 * (synchronising `stream`) whether the word of the last forward of shape (B, T, ragged) that
 * used `workspace` was set (diagnostics).  spk_model_forward_exact() (same arguments as
 * spk_model_forward_lengths, lengths may be NULL) runs the exact plan only.  A handle whose
 * packed weights leave fp16's range always runs exact.  The workspace queries cover both
 * plans. */
int spk_model_range_check(spk_model_t* model, int32_t B, int32_t T, int32_t ragged, const void* workspace,
                          void* stream, int32_t* overflowed);
int spk_model_forward_exact(spk_model_t* model, const float* feats, int32_t B, int32_t T, const int32_t* lengths,
                            void* workspace, size_t workspace_bytes, float* emb_out, void* stream);
/* How the guarded forward of shape (B, T, ragged) is cut (diagnostics, tests): the exact
 * re-run is captured per segment of the plan, right behind the segment it can replace, and
 * only for segments with a split-GEMM operand not statically bounded below 2^14 (ERes2Net*:
 * Hardtanh / weight-norm bounds leave only the stem's segment; ResNet: one segment, the whole
 * plan; ECAPA-TDNN / CAM++: scaled split, one segment, no twin).  n_segments: segments of the
 * plan; n_twin_segments: those with an exact twin; n_gated_steps: launches of the exact plan
 * enqueued behind every guarded forward (no-ops unless the range word is set); 0 / 0 / 0 for
 * an exact-only handle. */
int spk_model_guard_plan(spk_model_t* model, int32_t B, int32_t T, int32_t ragged, int32_t* n_segments,
                         int32_t* n_twin_segments, int32_t* n_gated_steps);

/* Algorithmic FLOPs per utterance of T frames (2 x conv/linear MACs). */
int spk_model_flops(spk_model_t* model, int32_t T, double* flops);

/* Introspection / measurement of the launch plan for a [B, T] batch: number of steps,
 * each step's name, the kernel it launches (rocprofv3 naming) and its algorithmic FLOPs;
 * spk_model_forward_timed() is spk_model_forward() with a HIP event around every step
 * (synchronises; used by bench.py for the roofline figure, not for throughput). */
int spk_model_plan_size(spk_model_t* model, int32_t B, int32_t T, int32_t* n_steps);
int spk_model_plan_step(spk_model_t* model, int32_t B, int32_t T, int32_t i, char* name, int32_t name_len,
                        char* kernel, int32_t kernel_len, double* flops);
/* Algorithmic HBM bytes of plan step i (every operand read / written once, fp32; conv
 * steps only, 0 for steps that are not priced): the byte side of the per-launch roofline. */
int spk_model_plan_step_bytes(spk_model_t* model, int32_t B, int32_t T, int32_t i, double* bytes);
int spk_model_forward_timed(spk_model_t* model, const float* feats, int32_t B, int32_t T, void* workspace,
                            size_t workspace_bytes, float* emb_out, void* stream, float* step_ms,
                            int32_t max_steps);

/* out[i*ldo + j] = <Ea_i, Eb_j> / (max(|Ea_i|,eps) * max(|Eb_j|,eps)), device pointers,
 * row-major [Na,E] and [Nb,E] float32.  Matches sklearn cosine_similarity (normalize with
 * zero-norm rows left as zero). */
int spk_cosine_affinity(const float* Ea, int64_t Na, const float* Eb, int64_t Nb, int32_t E, float* out,
                        int64_t ldo, void* stream);

/* Consumers of the cosine affinity, applied where each tile is produced (the N x Nb matrix is
 * never written): for every row i of Ea, the k best (score, column) pairs over Eb, ordered by
 * score descending then column ascending, and the number of columns with score >= threshold.
 * exclude_self drops column i + self_offset of row i (a rank's row block [r0, r1) of the
 * all-gathered embeddings: self_offset = r0).  Outputs (device, any may be NULL):
 * top_scores [Na][k] float32, top_index [Na][k] int64 (-1 when fewer than k columns),
 * count_ge [Na] int64.  workspace: device, spk_cosine_topk_workspace_bytes(Na, Nb). */
#define SPK_CONSUME_TOPK 1
typedef struct {
  int32_t kind;            /* SPK_CONSUME_TOPK */
  int32_t k;               /* 1..8 */
  int32_t exclude_self;
  int64_t self_offset;
  float threshold;
  float* top_scores;
  int64_t* top_index;
  int64_t* count_ge;
  void* workspace;
  size_t workspace_bytes;
} spk_affinity_consumer_t;
int spk_cosine_topk_workspace_bytes(int64_t Na, int64_t Nb, size_t* bytes);
int spk_cosine_topk(const float* Ea, int64_t Na, const float* Eb, int64_t Nb, int32_t E,
                    const spk_affinity_consumer_t* consumer, void* stream);

/* Trial scoring: scores[t] = cosine(Ea[ia[t]], Eb[ib[t]]) for n_trials (enrol, test) index
 * pairs (device int64 arrays), sklearn semantics (zero-norm rows divide by 1). */
int spk_cosine_trials(const float* Ea, const float* Eb, int32_t E, const int64_t* ia, const int64_t* ib,
                      int64_t n_trials, float* scores, void* stream);

/* Spectral clustering preparation (reference cluster.py SpectralCluster.p_pruning :64-77
 * and get_laplacian :79-84): S is the N x N cosine affinity (row stride lds); every row's
 * n_elems smallest entries are zeroed (ties at the threshold lowest index first), the
 * result symmetrised, its diagonal zeroed, and L = diag(row |sums|) - M written to L (row
 * stride ldl).  workspace: N*N floats (device). */
int spk_spectral_laplacian(const float* S, int64_t N, int64_t lds, int32_t n_elems, float* L, int64_t ldl,
                           void* workspace, size_t workspace_bytes, void* stream);

/* All eigenpairs of a symmetric N x N matrix (rocSOLVER ssyevd; replaces ARPACK eigsh in
 * cluster.py:88-89): eigenvalues ascending into w (device, N), eigenvector k overwrites row
 * k of A (row-major, stride lda).  Synchronises the stream. */
int spk_symmetric_eig(float* A, int64_t N, int64_t lda, float* w, void* stream);

/* Average-linkage AHC of an N x N cosine affinity (reference cluster.py:139-156): the flat
 * clusters fcluster(criterion='distance') cuts at -threshold, i.e. what is left when the two
 * clusters with the largest average pairwise similarity are merged until that value is below
 * threshold.  Ties go to the largest value, then the smallest row, then the smallest column; the
 * merged cluster keeps the smaller index.  S (device, row stride lds >= N, only its upper
 * triangle is read, like scipy's squareform) is not modified; labels (device, N) are numbered
 * by first occurrence (row 0's cluster is 0, the next new cluster 1, ...) and n_clusters (device,
 * 1) is their count.  N = 1 gives label 0.  The working matrix is fp64 and lives, with every other
 * piece of state, in the caller's workspace (device, 8-byte aligned, spk_ahc_workspace_bytes:
 * about 8 N^2 bytes).  Launches run on `stream`; the entry point synchronises it every 256 merge
 * steps to read whether the loop has finished.
 * Errors: N < 1, lds < N or a null pointer SPK_E_INVALID; a workspace below
 * spk_ahc_workspace_bytes(N) SPK_E_WORKSPACE; N above the cap of 32768 (an 8 GiB matrix)
 * SPK_E_UNSUPPORTED from both; a library built without the kernels SPK_E_UNSUPPORTED from
 * spk_ahc_average.  Nothing is written on an error. */
int spk_ahc_workspace_bytes(int64_t N, size_t* bytes);
int spk_ahc_average(const float* S, int64_t N, int64_t lds, float threshold, int32_t* labels, int32_t* n_clusters,
                    void* workspace, size_t workspace_bytes, void* stream);

/* The same clustering for n_prob independent affinities in one call, for short and multi-file
 * diarization: one workgroup per problem runs the whole merge loop inside a single launch, so the
 * launch count (two per 64 problems) does not depend on N, and nothing is read back: no host
 * synchronisation.  S, N, lds, threshold and labels are HOST arrays of n_prob entries; S[p]
 * (device, N[p] x N[p], row stride lds[p] >= N[p], not modified) and labels[p] (device, N[p]) are
 * device pointers, n_clusters is a device int32[n_prob].  Labels and counts of every problem are
 * those spk_ahc_average gives for it alone, to the bit, whatever the order of the problems.
 * Every N[p] must lie in [1, spk_ahc_batched_max_n()] (4096: the per-problem state lives in LDS);
 * the workspace (device, 8-byte aligned) holds one fp64 matrix per problem,
 * spk_ahc_average_batched_workspace_bytes (about 8 * sum N[p]^2).  n_prob == 0 succeeds and
 * launches nothing.
 * Errors, for the whole call and checked before anything is launched: a null pointer, n_prob < 0,
 * N[p] < 1 or lds[p] < N[p] SPK_E_INVALID; N[p] above the cap SPK_E_UNSUPPORTED (cluster that
 * problem with spk_ahc_average); a workspace too small SPK_E_WORKSPACE; a library built without
 * the kernels SPK_E_UNSUPPORTED from spk_ahc_average_batched.  Nothing is written on an error. */
int spk_ahc_batched_max_n(void);
int spk_ahc_average_batched_workspace_bytes(const int64_t* N, int32_t n_prob, size_t* bytes);
int spk_ahc_average_batched(const float* const* S, const int64_t* N, const int64_t* lds, const float* threshold,
                            int32_t n_prob, int32_t* const* labels, int32_t* n_clusters, void* workspace,
                            size_t workspace_bytes, void* stream);

/* Cohort score normalisation of trial scores (S-norm, and AS-norm, its adaptive top-N form).  The
 * reference has none; these entries replace what a user writes in numpy next to
 * compute_score_metrics.py today, for the enrol side (and likewise the test side):
 *     S = cosine_similarity(enrol, cohort)               # N x Nc, on the host
 *     top = -np.partition(-S, K - 1, axis=1)[:, :K]      # the K best cohort scores of every row
 *     mu, sd = top.mean(1), top.std(1)                   # ddof = 0
 *     score[t] = 0.5 * ((s[t] - mu_e[ia[t]]) / sd_e[ia[t]] + (s[t] - mu_t[ib[t]]) / sd_t[ib[t]])
 * K = Nc is S-norm.
 *
 * spk_topk_stats: mean[r] and std[r] (population, ddof = 0; device float32 [rows]) of the K largest
 * of S[r][0 .. cols) for a device float32 matrix with row stride lds >= cols; only [0, cols) of a
 * row is read.  The selection is exact: with v the K-th largest value of the row and g the number
 * of entries strictly above it, sum = (sum of the entries above v) + (K - g) v, and the squares
 * likewise, so equal values across the cut cannot change the result (-0.0 counts as +0.0).  Sums are
 * fp64 in a fixed order without float atomics (the same input gives the same bits), var =
 * max(sum2 / K - mean^2, 0).  K = 1 gives std 0.  Inputs are finite.
 *
 * spk_cosine_cohort_stats: the same statistics of the rows of the N x Nc cosine affinity of X
 * [N, E] against the cohort C [Nc, E] (spk_cosine_affinity's kernel and semantics), without that
 * matrix in memory at once: blocks of R rows are scored into the workspace and reduced in turn,
 * R the largest multiple of 128 the workspace holds (R * Nc * 4 bytes, at least one block of 128).
 * Rows are independent, so the result has the same bits for any workspace of at least min_bytes;
 * spk_cosine_cohort_stats_workspace_bytes also returns the recommended size (blocks of about
 * 128 MiB, which stay in the Infinity Cache between the passes of the selection).
 *
 * spk_cosine_trials_norm: spk_cosine_trials with the normalisation applied; s is the raw cosine of
 * the same device function, bit for bit, and
 *     scores[t] = 0.5f * ((s - mean_a[ia[t]]) / max(std_a[ia[t]], 1e-6f)
 *                         + (s - mean_b[ib[t]]) / max(std_b[ib[t]], 1e-6f))
 * in float32 (mean_a / std_a indexed like the rows of Ea, mean_b / std_b like those of Eb).  The
 * 1e-6 floor keeps a degenerate cohort (all of the K best scores equal) finite.
 *
 * All four only enqueue.  Errors: a null pointer, rows / cols / N / Nc / n_trials < 1, lds < cols,
 * K < 1, K > cols (K > Nc), E not a positive multiple of 4 SPK_E_INVALID; a workspace below
 * min_bytes SPK_E_WORKSPACE; cols, N or Nc above 2^31 - 1, or a library built without the kernels,
 * SPK_E_UNSUPPORTED.  Nothing is written on an error. */
int spk_topk_stats(const float* S, int64_t rows, int64_t cols, int64_t lds, int32_t K, float* mean, float* std,
                   void* stream);
int spk_cosine_cohort_stats_workspace_bytes(int64_t N, int64_t Nc, size_t* min_bytes, size_t* bytes);
int spk_cosine_cohort_stats(const float* X, int64_t N, const float* C, int64_t Nc, int32_t E, int32_t K, float* mean,
                            float* std, void* workspace, size_t workspace_bytes, void* stream);
int spk_cosine_trials_norm(const float* Ea, const float* Eb, int32_t E, const int64_t* ia, const int64_t* ib,
                           int64_t n_trials, const float* mean_a, const float* std_a, const float* mean_b,
                           const float* std_b, float* scores, void* stream);

/* Pair-cosine statistics of a ragged batch of embedding groups: the arithmetic of the reference's
 * speakerlab/bin/check_single_speaker.py (every segment pair's cosine, their minimum and mean) for
 * many files in one call.  X: device float32 [N_total, E], row stride ldx, 16-byte aligned rows;
 * offsets: HOST int64 [G + 1], offsets[0] = 0, non-decreasing; group g is rows offsets[g] ..
 * offsets[g + 1], n_g of them, P_g = n_g (n_g - 1) / 2 pairs.
 *
 * spk_pair_cosine_sizes (host arithmetic, no GPU needed): pair_offsets (HOST int64 [G + 1]), the
 * prefix sums of P_g.
 *
 * spk_pair_cosine_stats, outputs on the device:
 *   cos      float32 [pair_offsets[G]] or NULL: group g's pair cosines at cos[pair_offsets[g] ..], in
 *            condensed upper-triangle row-major order (0,1), (0,2), ..., (1,2), ... (the order of
 *            np.triu_indices(n, 1)); each is the value, bit for bit, spk_cosine_trials gives for the
 *            two rows (sklearn semantics, a zero-norm row divides by 1 and scores 0);
 *   min      float32 [G]; argmin int64 [G]: the condensed index of the minimum inside the group,
 *            the smallest one among equal values;
 *   mean     float32 [G]: the fp64 sum of the fp32 cosines, in an order fixed by the pairs' condensed
 *            indices alone, divided by P_g and rounded once;
 *   n_below  int64 [G]: pairs with cosine < threshold (strictly);
 *   a group with n_g <= 1: min = mean = 1.0 (the reference's rule), argmin = -1, n_below = 0.
 *   a NaN cosine (a non-finite row) orders below every number: min is NaN, argmin the first NaN,
 *   the mean NaN, as numpy's min / argmin / mean of the cosines; it is never below the threshold.
 * A group's outputs have the same bits alone and inside any batch, with and without cos.  With cos
 * the pairs are scored by one wave each across the device, in launches of at most 2^25 pairs (a
 * grid is a 32-bit count of work-items, and a pair takes a wave), and a workgroup per group reduces
 * them; with cos == NULL one workgroup per group does both, which suits the tool's groups of tens
 * of rows and is capped at 4096 rows per group.  Enqueues only (the offsets travel as kernel
 * arguments, 64 groups per launch).  G == 0 succeeds and launches nothing; without any pair only
 * the statistics' launch runs.
 * Errors, all checked before the first launch: a null pointer (cos excepted; X only when there are
 * rows), G < 0, E not a positive multiple of 4, ldx < E or not a multiple of 4, an X that is not
 * 16-byte aligned, offsets[0] != 0 or decreasing offsets SPK_E_INVALID; a group above the cap of
 * 32768 rows (4096 with cos == NULL), or a library built without the kernels, SPK_E_UNSUPPORTED.
 * Nothing is written on an error.
 *
 * spk_pair_cosine_plan (host arithmetic, diagnostics and tests): the launches spk_pair_cosine_stats
 * makes for these offsets, from the plan it walks itself: the number of pair launches (0 without
 * cos) and of statistics launches, the most pairs one pair launch covers, and the pairs all of
 * them cover together (pair_offsets[G] with cos). */
int spk_pair_cosine_sizes(const int64_t* offsets, int32_t G, int64_t* pair_offsets);
int spk_pair_cosine_stats(const float* X, int64_t ldx, int32_t E, const int64_t* offsets, int32_t G, float threshold,
                          float* cos, float* min, float* mean, int64_t* argmin, int64_t* n_below, void* stream);
int spk_pair_cosine_plan(const int64_t* offsets, int32_t G, int32_t with_cos, int64_t* n_pair_launches,
                         int64_t* n_stats_launches, int64_t* max_launch_pairs, int64_t* planned_pairs);

/* Corpus similarity statistics: what the reference's
 * egs/extract_and_comclude_similarities/compute_speaker_similarities_fast.py takes from the N x N
 * cosine matrix of one embedding set X [N, E] (device float32, contiguous, 16-byte aligned), without
 * that matrix ever existing.  Score (i, j) is, bit for bit, the value spk_cosine_affinity(X, X)
 * writes at [i][j] (sklearn semantics: a zero-norm row divides by 1).  As in
 * spk_cosine_cohort_stats, blocks of R rows against all N columns are scored into the caller's
 * workspace and consumed in turn, R the largest multiple of 128 the workspace holds.
 * spk_cosine_sim_workspace_bytes gives the smallest workspace (128 * N * 4 bytes), the recommended
 * one (blocks of about 128 MiB, which stay in the Infinity Cache between the kernel that writes
 * them and the ones that read them) and the size of the triangle entries' device state (their
 * counters, tables and collected pairs; 16-byte aligned, contents undefined between calls).  Every
 * result has the same bits for every workspace from the smallest up.  No float atomics; every fp64
 * sum has a fixed order (csrc/sim_stats.hip).  -0.0 and +0.0 are one value throughout and are
 * reported as +0.0.
 *
 * spk_cosine_rows_topk, outputs on the DEVICE, enqueues only.  Per row i, over the columns j != i:
 *   top_scores float32 [N][k], top_index int64 [N][k]: the k best, score descending then column
 *              ascending; -inf / -1 from position N - 1 on where N - 1 < k.  k in 1..1024.
 *   sum, sumsq double [N]; min, max float32 [N] (NaN for N == 1); self float32 [N] = score (i, i).
 *
 * spk_cosine_triu_stats and spk_cosine_triu_hist, over the P = N (N - 1) / 2 pairs i < j, each taken
 * from row i.  Their small inputs and all their outputs are HOST memory, and both SYNCHRONISE the
 * stream: spk_cosine_triu_stats once per pass of its select (the bins are picked on the host),
 * spk_cosine_triu_hist once at its end.  Together they make at most five passes over the scores.
 * spk_cosine_triu_stats:
 *   count int64 = P; sum, sumsq double; min, max float32;
 *   count_ge int64 [n_thr]: pairs with score >= thresholds[t], compared in float32; n_thr <= 32;
 *   order_stats float32 [n_ranks]: the exact order statistics at the 0-based ascending ranks
 *              (ascending, below P; n_ranks <= 16), by one multi-target MSB-first radix select of
 *              four 8-bit digit passes, the first one in the same pass as the moments;
 *   ext_cut float32 [2], ext_take int32 [2]: for n_eff = min(n_ext, P) > 0 the score of the n_eff-th
 *              largest and of the n_eff-th smallest pair, and how many copies of that score belong to
 *              the n_eff; two more targets of the same select.  n_ext <= 4096; NaN / 0 for n_ext == 0.
 *   N == 1: count 0, sum, sumsq, min, max NaN, cuts NaN / 0; nothing is launched.
 * spk_cosine_triu_hist, one pass:
 *   hist int64 [nbins] over edges double [nbins + 1] (finite, ascending; nbins <= 256): bin b holds the
 *              pairs with edges[b] <= (double)s < edges[b + 1], the last bin also s == edges[nbins];
 *   with n_ext > 0 and ext_cut / ext_take as spk_cosine_triu_stats gave them for the same X and n_ext:
 *   ext_scores float32 [2][n_ext], ext_i, ext_j int64 [2][n_ext], n_found int32 [2]: row 0 the n_found[0]
 *              = n_eff largest pairs, score descending then (i, j) ascending; row 1 the n_eff smallest,
 *              score ascending then (i, j) ascending.  Among equal scores at a cut the first in (i, j)
 *              order are taken.  Entries from n_found on are not written.
 *
 * Errors, all checked before the first launch, nothing written: a null pointer, N < 1, E not a
 * positive multiple of 4, an X that is not 16-byte aligned, k or n_ext, n_thr, n_ranks, nbins out of
 * range, a NaN threshold, ranks not ascending or at or above P (so any rank with N == 1), edges not
 * ascending, cuts that cannot be spk_cosine_triu_stats's SPK_E_INVALID; a workspace below min_bytes or
 * a state below state_bytes SPK_E_WORKSPACE; N above 2^31 - 1, an N whose single tile of rows would
 * be a launch of 2^31 work-items or more, or a library built without the kernels
 * SPK_E_UNSUPPORTED.  spk_cosine_triu_hist also answers SPK_E_INVALID, after its pass and with
 * nothing written, when the pairs beyond the cuts are not n_eff - ext_take. */
int spk_cosine_sim_workspace_bytes(int64_t N, size_t* min_bytes, size_t* bytes, size_t* state_bytes);
int spk_cosine_rows_topk(const float* X, int64_t N, int32_t E, int32_t k, float* top_scores, int64_t* top_index,
                         double* sum, double* sumsq, float* min, float* max, float* self, void* workspace,
                         size_t workspace_bytes, void* stream);
int spk_cosine_triu_stats(const float* X, int64_t N, int32_t E, const float* thresholds, int32_t n_thr,
                          const int64_t* ranks, int32_t n_ranks, int32_t n_ext, int64_t* count, double* sum,
                          double* sumsq, float* min, float* max, int64_t* count_ge, float* order_stats, float* ext_cut,
                          int32_t* ext_take, void* workspace, size_t workspace_bytes, void* state, size_t state_bytes,
                          void* stream);
int spk_cosine_triu_hist(const float* X, int64_t N, int32_t E, const double* edges, int32_t nbins, int32_t n_ext,
                         const float* ext_cut, const int32_t* ext_take, int64_t* hist, float* ext_scores,
                         int64_t* ext_i, int64_t* ext_j, int32_t* n_found, void* workspace, size_t workspace_bytes,
                         void* state, size_t state_bytes, void* stream);

/* All-pairs verification statistics: what exact EER / minDCF / AUC over every labelled pair of one
 * embedding set need, without the N x N matrix ever existing.  X [N, E] as for the corpus similarity
 * statistics above (device float32, contiguous, 16-byte aligned), labels int32 [N] on the DEVICE, the
 * speaker index of each row, none negative.  Pair (i, j), i < j, taken from row i, has class 1 (target)
 * when labels[i] == labels[j] and class 0 (non-target) otherwise; its score is, bit for bit, what
 * spk_cosine_affinity(X, X) writes at [i][j], and its key is the order-preserving 32-bit image of
 * that float (bits b: b == 0x80000000 -> 0 first, so -0.0 and +0.0 share a key; then ~b when the sign
 * bit is set, b | 0x80000000 otherwise).  The row blocking, the workspace sizes and their meaning
 * are those of spk_cosine_sim_workspace_bytes; state_bytes is the size of these entries' own device
 * state (16-byte aligned, contents undefined between calls).  Small inputs and all outputs are HOST
 * memory; each entry makes one pass over the scores and SYNCHRONISES the stream twice (once for
 * the labels' check, once at its end).  All counts are exact integers, every result has the same
 * bits for every workspace from the smallest up, no float atomics, fp64 sums in the fixed order of
 * csrc/verif_stats.hip.
 *
 * spk_cosine_verif_moments, per class c:
 *   count int64 [2]; sum, sumsq double [2] (0 for an empty class); min, max float32 [2], NaN for an
 *   empty class;
 *   hist int64 [2][nbins] over edges double [nbins + 1] (finite, ascending; nbins <= 256, 0: none), bin
 *              semantics exactly those of spk_cosine_triu_hist.
 *   N == 1: counts 0, sums, min, max NaN, hist 0; nothing is launched.
 * spk_cosine_verif_digits, the primitive of the exact searches:
 *   level in 0..3 and prefixes uint32 [n_prefix], n_prefix in 1..16, of which only the top `level`
 *              bytes count (level 0: one empty prefix, n_prefix == 1, prefixes may be null);
 *   digits int64 [n_prefix][2][256]: digits[p][c][d] = the class-c pairs whose key agrees with
 *              prefix p in its top `level` bytes and whose next byte is d.  Equal prefixes get equal
 *              rows.  N == 1: zeros.
 *
 * Errors: a null pointer, N < 1, E not a positive multiple of 4, an X that is not 16-byte aligned,
 * nbins, level or n_prefix out of range, edges not finite and ascending, a negative label (found by
 * a kernel before the pass, nothing written) SPK_E_INVALID; a workspace below min_bytes or a state
 * below state_bytes SPK_E_WORKSPACE; N above 2^31 - 1, an N whose single tile of rows would be a
 * launch of 2^31 work-items or more, or a library built without the kernels SPK_E_UNSUPPORTED. */
int spk_cosine_verif_workspace_bytes(int64_t N, size_t* min_bytes, size_t* bytes, size_t* state_bytes);
int spk_cosine_verif_moments(const float* X, const int32_t* labels, int64_t N, int32_t E, const double* edges,
                             int32_t nbins, int64_t* count, double* sum, double* sumsq, float* min, float* max,
                             int64_t* hist, void* workspace, size_t workspace_bytes, void* state, size_t state_bytes,
                             void* stream);
int spk_cosine_verif_digits(const float* X, const int32_t* labels, int64_t N, int32_t E, int32_t level,
                            const uint32_t* prefixes, int32_t n_prefix, int64_t* digits, void* workspace,
                            size_t workspace_bytes, void* state, size_t state_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SPK_HIP_H */
