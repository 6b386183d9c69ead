/*
 * llama2_q4.h -- C ABI of the MI355X-native llama2_q4 decode path (libllama2_q4.so).
 *
 * The reference (ankan-ban/llama_cu_awq) has no plugin/FFI layer: it is one CUDA translation
 * unit whose host functions launch kernels on a file-scope stream.  The drop-in boundary is
 * therefore source-level: the same structs (common.h:9-78) and the same host entry points
 * (llama2_q4.cu:209-432, sampler.h:15-82), exported here as `extern "C"` functions over plain
 * pointers and sizes.  Differences forced by a C ABI, and nothing else:
 *   - `half*`  -> `q4_half*` (uint16_t bit pattern of an IEEE binary16),
 *   - `QWeight&` -> `const QWeight*`,
 *   - the file-scope `cudaStream_t stream` (llama2_q4.cu:207) -> `q4_set_stream()/q4_get_stream()`,
 *   - `printf + exit(EXIT_FAILURE)` -> a non-zero return code (the C++ wrappers in
 *     llama2_q4.hpp turn it back into the reference's message + exit), see q4_status.
 * Every declaration cites the reference interface it replaces (file:line in /root/reference).
 *
 * All device pointers are HIP device pointers (hipMalloc) unless stated otherwise.  All launchers
 * enqueue on the current q4 stream and return without synchronising, like the reference.
 */
#ifndef LLAMA2_Q4_H
#define LLAMA2_Q4_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef uint16_t q4_half;          /* fp16 bits (reference: CUDA `half`) */
typedef void* q4_stream_t;         /* hipStream_t */

enum { Q4_MAX_SEQ_LEN_SMEM_KERNEL = 8192,      /* common.h:6 */
       Q4_MAX_SEQ_LEN = 128 * 1024,            /* common.h:7 */
       Q4_GROUP_SIZE = 128,                    /* llama2_q4.cu:31 */
       Q4_MAX_GRAPHS = 8 };                    /* llama2_q4.cu:342 */

typedef enum {
    Q4_OK = 0,
    Q4_ERR_UNSUPPORTED_SIZE = 1,   /* "Unsupported matmul size. Exiting" llama2_q4.cu:215,225,236,251 */
    Q4_ERR_ALLOC = 2,              /* "malloc failed..." llama2_q4.cu:53-58,62-65,129-133 */
    Q4_ERR_IO = 3,                 /* "Couldn't open file" / "Invalid header size" / "error reading weights" :158,412,414 */
    Q4_ERR_HIP = 4,                /* a HIP runtime call failed (the reference never checks) */
    Q4_ERR_ARG = 5,
    Q4_NOT_ADMITTED = 6            /* q4_verify_tokens only: nothing ran; run steps instead */
} q4_status;

const char* q4_status_string(int status);
const char* q4_last_error(void);   /* text of the last failing HIP call, "" if none */

/* ---- common.h:9-18 -- also the 32-byte file header, fread raw (llama2_q4.cu:414) ---------- */
typedef struct {
    int dim;          /* transformer dimension */
    int hidden_dim;   /* for ffn layers */
    int n_layers;
    int n_heads;      /* number of query heads */
    int n_kv_heads;   /* number of key/value heads */
    int vocab_size;
    int seq_len;      /* max sequence length */
    float rope_theta;
} Config;

/* ---- common.h:20-24.  Column-major per output column n, K = input length:
 *   weight[n*(K/8) + k/8]  nibble k%8 (LSB first) = q in [0,15]
 *   zeros [n*pzh   + g/8]  nibble g%8, g = k/128, pzh = divUp(divUp(K,128),8)
 *   scales[n*G     + g]    fp16,     G = divUp(K,128)                       (llama2_q4.cu:82-98) */
typedef struct {
    uint32_t* weight;
    uint32_t* zeros;
    q4_half* scales;
} QWeight;

/* common.h:26-36 */
typedef struct {
    q4_half* rms_att_weight;
    q4_half* rms_ffn_weight;
    QWeight wq_q, wq_k, wq_v, wq_o, wq_gate, wq_up, wq_down;
} PerLayerWeight;

/* common.h:38-48 */
typedef struct {
    q4_half* token_embedding_table;   /* (vocab_size, dim) */
    q4_half* wcls;                    /* (vocab_size, dim), not quantised */
    q4_half* rms_final_weight;        /* (dim,) */
    PerLayerWeight* layers;           /* host array of device pointers */
    int num_layers;
} TransformerWeights;

/* common.h:51-54 -- pinned, device-mapped host memory (hipHostMalloc) */
typedef struct {
    volatile int pos;
    int tokens[Q4_MAX_SEQ_LEN];
} SharedData;

/* common.h:56-72, same fields in the same order */
typedef struct {
    q4_half* x;            /* (dim,)   fp16 residual stream */
    q4_half* xb;           /* (dim,) */
    q4_half* hb;           /* (hidden_dim,) */
    q4_half* q;            /* (dim,) */
    q4_half* att;          /* (n_heads, seq_len) scratch; this build's attention keeps scores on chip and
                              uses it only for split-context partials */
    q4_half* logits;       /* (vocab_size,) */
    q4_half* key_cache;    /* (layer, seq_len, kv_dim) */
    q4_half* value_cache;  /* (layer, seq_len, kv_dim) */
    int* pos;              /* device copy of the current position */
    SharedData* shared_data;
    float* logits_array;   /* (seq_len, vocab_size) fp32, perplexity mode only */
} RunState;

/* common.h:74-78 */
typedef struct {
    Config config;
    TransformerWeights weights;
    RunState state;
} Transformer;

/* sampler.h:3-13 */
typedef struct {
    int vocab_size;
    int* indices;
    void* tempStorage_scan;
    void* tempStorage_sort;
    size_t temp_storage_bytes_scan;
    size_t temp_storage_bytes_sort;
    float temperature;
    float topp;
    unsigned long long rng_state;
} Sampler;

/* ---- stream (replaces the file-scope `cudaStream_t stream`, llama2_q4.cu:207,700) ---------- */
int q4_set_device(int device);
int q4_stream_create(q4_stream_t* out);          /* cudaStreamCreate, llama2_q4.cu:700 */
/* a stream restricted to the first n_cus compute units (hipExtStreamCreateWithCUMask): replicas side by side on one GPU.
 * Fusion level 3 counts the waiting blocks of ITS launch against the CUs of ITS stream (the forward-progress guard): models that
 * decode concurrently on one GPU at level 3 must use streams with DISJOINT CU masks (or level 1); two unmasked streams can fill
 * every CU with each other's waiting blocks, which ends as bounded time-outs and a drop to level 1, never as a hang. */
int q4_stream_create_masked(q4_stream_t* out, int n_cus);
int q4_stream_destroy(q4_stream_t s);
void q4_set_stream(q4_stream_t s);
q4_stream_t q4_get_stream(void);
int q4_stream_synchronize(void);                 /* cudaStreamSynchronize(stream), llama2_q4.cu:468 */
int q4_device_synchronize(void);                 /* cudaDeviceSynchronize, perplexity.h:81 */

/* ---- device memory helpers for callers that own buffers (tests, benches, other hosts) -------- */
int q4_malloc(void** dptr, size_t bytes);
int q4_free(void* dptr);
int q4_memcpy_h2d(void* dst, const void* src, size_t bytes);
int q4_memcpy_d2h(void* dst, const void* src, size_t bytes);
int q4_memset(void* dst, int value, size_t bytes);

/* ---- device kernels' launchers (llama2_q4.cu:209-284) ------------------------------------- */

/* rmsnorm(half* o, half* x, half* weight, int size)  llama2_q4.cu:209-212, kernel gpu_kernels.h:72-105 */
int q4_rmsnorm(q4_half* o, const q4_half* x, const q4_half* weight, int size);

/* matmul(half* xout, half* x, half* w, int n, int d, int batch, int x_stride, int w_stride, int op_stride,
 *        int w_row_stride, float alpha)  llama2_q4.cu:214-222, kernel mat_vec_kernel gpu_kernels.h:109-139.
 * fp16 GEMV: xout[b][i] = alpha * sum_j w[b*w_stride + i*w_row_stride + j] * x[b*x_stride + j].
 * w_row_stride == -1 means n. */
int q4_matmul_f16(q4_half* xout, const q4_half* x, const q4_half* w, int n, int d, int batch, int x_stride,
                  int w_stride, int op_stride, int w_row_stride, float alpha);

/* matmul(half* xout, half* x, QWeight& w, int inpSize, int opSize, bool accum, int loff, int* pPos)
 * llama2_q4.cu:224-233, kernel mat_vec_kernel_int4 gpu_kernels.h:213-240 (+ get_mat_vec_int4 :171-210).
 * accum: xout = half(float(xout) + sum).  loff != -1: xout += loff + *pPos * opSize (KV-cache addressing). */
int q4_matmul_q4(q4_half* xout, const q4_half* x, const QWeight* w, int inpSize, int opSize, int accum,
                 int loff, const int* pPos);

/* qkv_matvec(...) llama2_q4.cu:235-248, kernel qkv_matvec_kernel gpu_kernels.h:242-254 */
int q4_qkv_matvec(q4_half* q, q4_half* key_cache, q4_half* value_cache, const q4_half* x, const QWeight* qw,
                  const QWeight* kw, const QWeight* vw, int inpSize, int opSize, int loff, const int* pPos);

/* ffn_matvec_silu(...) llama2_q4.cu:250-261, kernel ffn_matvec_silu_kernel gpu_kernels.h:256-275 */
int q4_ffn_matvec_silu(q4_half* xout, const q4_half* x, const QWeight* gate_w, const QWeight* up_w, int inpSize,
                       int opSize);

/* RoPERotation(half* q, half* k, int num_heads, int num_kv_heads, int head_size, int* pPos, int loff,
 *              float rope_theta)  llama2_q4.cu:263-265, kernel gpu_kernels.h:332-355.  k = key cache base. */
int q4_rope_rotation(q4_half* q, q4_half* k, int num_heads, int num_kv_heads, int head_size, const int* pPos,
                     int loff, float rope_theta);

/* MultiHeadAttention(half* output, half* q, half* key_cache, half* value_cache, half* att, int num_heads,
 *                    int head_size, int kv_mul, int max_seq_len, int* pPos)  llama2_q4.cu:267-284
 * (kernels mat_vec_kernel_simple :142-168, softmax_kernel :357-446, vec_mat_kernel :279-329).
 * key_cache/value_cache already offset by loff.  One flash-decode kernel here: scores never leave the CU. */
int q4_multi_head_attention(q4_half* output, const q4_half* q, const q4_half* key_cache,
                            const q4_half* value_cache, q4_half* att, int num_heads, int head_size, int kv_mul,
                            int max_seq_len, const int* pPos);
/* The same over FP8 (OCP e4m3fn) caches, the layout of Q4_KV_FP8 models: k8 / v8 [max_seq_len][kv_dim] bytes, k_exp / v_exp
 * [n_kv_heads][max_seq_len] signed row exponents (a row of one position and kv head is head_size bytes times 2^e, e the smallest integer
 * in [-15, 7] with amax <= 448 * 2^e). k_row / v_row [kv_dim] halves hold position *pPos (K already rotated): the launch quantises them,
 * attends over their round trip and APPENDS bytes and exponents at *pPos; it reads no cache row at or past *pPos. Head sizes 64, 128, 256.
 * att: null (one block per head at any context), or a scratch of at least 8 * num_heads * max_seq_len BYTES: bins from 512 positions then run one block per
 * (head, chunk) with flash-decode records in it, merged by a second launch. */
int q4_multi_head_attention_kv8(q4_half* output, const q4_half* q, uint8_t* k8, uint8_t* v8, int8_t* k_exp, int8_t* v_exp,
                                const q4_half* k_row, const q4_half* v_row, q4_half* att, int num_heads, int head_size, int kv_mul,
                                int max_seq_len, const int* pPos);

/* copy_embedding_kernel gpu_kernels.h:61-69, launch llama2_q4.cu:294. tokens: device-visible int array */
int q4_copy_embedding(q4_half* x, const q4_half* table, int size, const int* tokens, const int* pPos);

/* convert_fp16_to_fp32 gpu_kernels.h:55-59, launch llama2_q4.cu:381 */
int q4_convert_fp16_to_fp32(float* out, const q4_half* in, int elements);

/* argmax_kernel gpu_kernels.h:448-493 (launch sampler.h:49). result: token ring (device-visible),
 * pPos: host-visible position (SharedData::pos), pPosGpu: device position. Ties -> lowest index. */
int q4_argmax(const q4_half* x, int size, int* result, volatile int* pPos, int* pPosGpu, int write_token);

/* Not in the reference: log-probabilities under the model's OWN distribution -- temperature 1, no nucleus; NOT the tempered / truncated distribution
 * the sampler draws from. logits: n >= 1 fp16 values (16-byte aligned). lse[0] = m + log(sum_i exp(l_i - m)), m the maximum, in fp32 (expf / logf, a
 * fixed summation order: the same input gives the same bits on every launch). top_ids / top_logprobs [top_k]: the top_k entries of highest logit,
 * ordered by (logit descending, index ascending) -- argmax_kernel's tie rule, entry 0 is the greedy token -- with their log-probabilities l - lse;
 * the order is exact on the halves (-0 equals +0; -inf contributes 0 and ranks last; a NaN ranks behind everything and makes lse NaN, never a
 * fault). target: null, or a device-visible int; *target in [0, n) writes target_logprob[0] = l_target - lse, else NaN. All pointers are device
 * pointers; enqueues on the q4 stream. top_k in [0, Q4_MAX_TOP_LOGPROBS], top_k > n is Q4_ERR_ARG; a vocabulary beyond about 300,000 entries at
 * top_k 20 (more at a smaller top_k) is Q4_ERR_UNSUPPORTED_SIZE. */
enum { Q4_MAX_TOP_LOGPROBS = 20 };
int q4_logprob_topk(const q4_half* logits, int n, int top_k, const int* target, float* lse, float* target_logprob, int* top_ids,
                    float* top_logprobs);
/* The row form of the same launch, for tests and tools: one block per row, n_rows rows (1 .. 8) of n halves, `ld` halves apart (ld a multiple of 8 and
 * >= n: rows stay 16-byte aligned; the halves between n and ld are neither read nor written). Row r's outputs -- lse[r], target_logprob[r], top_ids and
 * top_logprobs [r][top_k] -- are, byte for byte, what q4_logprob_topk writes for that row alone; targets: NULL, or [n_rows] device-visible ints. This is
 * the launch prompt and verify passes run with q4_set_pass_logprobs on. Errors: q4_logprob_topk's, plus Q4_ERR_ARG for n_rows outside 1 .. 8 and for an
 * ld below n or not a multiple of 8. */
int q4_logprob_topk_rows(const q4_half* logits, int ld, int n, int n_rows, int top_k, const int* targets, float* lse, float* target_logprob, int* top_ids,
                         float* top_logprobs);

/* ---- network + per-token step ------------------------------------------------------------- */

/* run_llama_network(int* pPos, Config*, RunState*, TransformerWeights*, int seq_len_bin) llama2_q4.cu:286-340 */
int q4_run_llama_network(const int* pPos, const Config* p, RunState* s, const TransformerWeights* w,
                         int seq_len_bin);

/* run_transformer(bool gen_token, Config*, RunState*, TransformerWeights*, bool copyLogits, Sampler*)
 * llama2_q4.cu:346-395: graph bin select / capture-once / replay, optional fp32 logits copy, sample(). */
int q4_run_transformer(int gen_token, const Config* p, RunState* s, const TransformerWeights* w, int copyLogits,
                       Sampler* pSampler);

/* run_transformer with the position supplied by the caller (SharedData::pos is not read back), so that step pos+1
 * can be queued while step pos runs; q4_wait_pos spins on SharedData::pos ("unblocks the CPU", gpu_kernels.h:490)
 * until the device has published position >= pos. generate() uses the pair instead of cudaStreamSynchronize
 * + run_transformer (llama2_q4.cu:468-470): same device order, no idle gap between tokens. */
int q4_run_transformer_at(int pos, int gen_token, const Config* p, RunState* s, const TransformerWeights* w,
                          int copyLogits, Sampler* pSampler);
int q4_wait_pos(const RunState* s, int pos);
/* Greedy steps need nothing from the host between tokens (the device keeps the position and feeds itself the ring), so a
 * token loop may queue Q4_MULTI_STEPS of them as ONE graph replay (sampled steps too: topp_sample_kernel is part of the graph and
 * takes its coin from a device ring by position, filled by the host from the sampler's xorshift stream before the replay): q4_steps_that_fit says how many steps (Q4_MULTI_STEPS or
 * 1) may go out at `pos` -- same gen_token for the whole group, one sequence-length bin, within `steps` --, and
 * q4_run_transformer_steps queues them (nsteps = 1 is q4_run_transformer_at). generate() uses the pair. */
enum { Q4_MULTI_STEPS = 8 };
int q4_steps_that_fit(int pos, int num_prompt_tokens, int steps, const Config* p, const Sampler* sampler);
int q4_run_transformer_steps(int pos, int nsteps, int gen_token, const Config* p, RunState* s, const TransformerWeights* w,
                             int copyLogits, Sampler* pSampler);

/* 0: 1:1 kernel sequence of the reference (10 launches/layer); 1: fused kernels (rmsnorm folded into the consumer GEMV,
 * RoPE + KV write in the QKV epilogue: 5 launches/layer); 3: additionally attention -> o-proj (llama2_q4.cu:320-323)
 * as ONE launch where the geometry has that form (heads of 64 / 128 / 256, multi-head or grouped-query) and every block of the
 * launch fits the stream's CUs at once: the o-proj blocks pull their weights while the heads work and take the heads' output
 * inside the launch (bounded waits, q4_handoff_status), 4 launches/layer. 2 selects 1 (round 2's QKV -> attention -> o-proj
 * launch was measured slower than level 1 and removed). Levels 1 and 3 run the same arithmetic with another fp32 grouping of an
 * attention output's positions (below bin 512 the fused launch's attention role takes 16 positions per wave instruction of a
 * 64-byte V slice, the stand-alone kernel 4; 8 waves instead of 16): logits agree within the model's tolerance in every bin, not
 * bit for bit. After a timed-out hand-off the library runs level 1 for the next 16 sequences (32, 64, ... after further
 * time-outs), then tries the level it had again; q4_set_fusion(level) re-arms it at once. Resets captured graphs.
 * 4: additionally the FFN half of a layer (rmsnorm + gate/up + SiLU + down projection + residual add, llama2_q4.cu:326-332) as ONE
 * launch where q4_ffn_pair_covers says so (Llama-2-7B's dim / hidden_dim): one block per CU computes its slice of hb, hands it to every
 * other CU inside the launch and multiplies its columns of the down projection, whose weights it has meanwhile streamed into LDS;
 * 3 launches/layer, bit-identical to levels 1 / 3 (same bounded waits, same fallback after a time-out).
 * 5 (default): that launch also runs rmsnorm + q/k/v + RoPE + KV write of the NEXT layer (llama2_q4.cu:300-317) as its third phase, on
 * weights it streams into LDS while it multiplies the down projection -- multi-head models of Llama-2-7B's shape; 2 launches/layer (the
 * first layer keeps its own QKV launch, the last layer's FFN half runs as at level 4), bit-identical as well.
 * 6 (opt-in; measured 1-2 % SLOWER than 5): below the split-context bins that launch also begins with THIS layer's attention and
 * output projection (llama2_q4.cu:320-323) -- half of its blocks run the attention role's (head, V slice) units, the other half the output
 * projection; the whole layer behind its q / k / v is ONE launch, 1 launch/layer; bit-identical to levels 3 / 4 / 5. */
void q4_set_fusion(int level);
int q4_get_fusion(void);
/* The K / V cache format of the models q4_build_transformer builds from now on (a model's format is fixed at build time): Q4_KV_FP16 (default:
 * every launch and every bit as without this call) or Q4_KV_FP8 -- e4m3 bytes with one exponent byte per (position, kv head), half the cache's
 * bytes; attention then is the fp16 attention over rows replaced by their FP8 round trip. Head sizes 64, 128 and 256; a build
 * with another fails with Q4_ERR_UNSUPPORTED_SIZE and a q4_last_error text. Returns Q4_ERR_ARG for any other value. */
enum { Q4_KV_FP16 = 0, Q4_KV_FP8 = 1 };
int q4_set_kv_format(int format);
int q4_get_kv_format(void);
/* the format of the model that owns this RunState; Q4_KV_FP16 for a RunState the library did not build */
int q4_kv_format_of(const RunState* s);
/* RoPE scaling of the models q4_build_transformer builds from now on (process-wide and read by the build, like q4_set_kv_format; a model's scaling is
 * fixed at build time; the 32-byte file header has no room for it). Q4_ROPE_NONE (default): the angles are pos / powf(rope_theta, 2i / head_size), every
 * launch and every bit as without this call. Otherwise the model gets head_size/2 per-pair frequencies inv_freq[i], computed in double and rounded once to
 * float: with f_i = pow((double)rope_theta, -(2.0 * i) / head_size),
 *   Q4_ROPE_LINEAR (position interpolation, Hugging Face rope_scaling type "linear"): f_i / factor;
 *   Q4_ROPE_LLAMA3 (Llama-3.1 / 3.2, Hugging Face _compute_llama3_parameters): with wl = 2 pi / f_i and orig = original_max_position,
 *     wl < orig / high_freq_factor keeps f_i, wl > orig / low_freq_factor gives f_i / factor, otherwise with
 *     s = (orig / wl - low_freq_factor) / (high_freq_factor - low_freq_factor) the result is (1 - s) * f_i / factor + s * f_i;
 *   Q4_ROPE_CUSTOM: the given floats as they are (per-pair factor lists, frequencies of another theta); n_freqs != head_size / 2 fails the build with
 *     Q4_ERR_ARG and a q4_last_error text.
 * The model's rotation table [seq_len][head_size/2] then holds (cosf(a), sinf(a)) of a = (float)pos * inv_freq[i], one fp32 multiply, and everything that
 * rotates reads it (fusion level 0 computes the same bits from the device copy of inv_freq): no launch is added to or changed in the decode step. For such
 * a model the table is mandatory -- a failed allocation is Q4_ERR_ALLOC, a table above 2^30 entries Q4_ERR_UNSUPPORTED_SIZE, never a fall-back to unscaled
 * angles. LINEAR with factor 1 is not the NONE path: its frequencies may differ from 1 / powf in the last bit. FP8 models, snapshots (a scaled model's
 * fingerprint also covers its frequencies) and context shift work as for any model. Not covered: YaRN / longrope (an attention factor), dynamic NTK. */
enum { Q4_ROPE_NONE = 0, Q4_ROPE_LINEAR = 1, Q4_ROPE_LLAMA3 = 2, Q4_ROPE_CUSTOM = 3, Q4_ROPE_MAX_PAIRS = 256 };
typedef struct {
    int kind;
    float factor;                 /* LINEAR, LLAMA3: finite, >= 1 */
    float low_freq_factor;        /* LLAMA3: finite, > 0, < high_freq_factor */
    float high_freq_factor;
    int original_max_position;    /* LLAMA3: >= 1 */
    int n_freqs;                  /* CUSTOM: head_size / 2, 1 .. Q4_ROPE_MAX_PAIRS */
    const float* inv_freq;        /* CUSTOM: host array, copied; each finite and >= 0 */
} q4_rope_scaling;
/* NULL or kind NONE: off. Q4_ERR_ARG: anything above violated or an unknown kind; nothing changes, no GPU touched. Fields the kind does not use are ignored. */
int q4_set_rope_scaling(const q4_rope_scaling* s);
int q4_get_rope_scaling(q4_rope_scaling* out);        /* inv_freq points at the library's copy (CUSTOM), else NULL */
/* the scaling of a built model (inv_freq: the model's own frequency array, whatever the kind; NULL for an unscaled model). Q4_ERR_ARG: a Transformer the
 * library did not build */
int q4_rope_scaling_of(const Transformer* t, q4_rope_scaling* out);
/* "none" | "linear,factor=4" | "llama3,factor=8,low=1,high=4,orig=8192": the kind first, then its keys, all of them, in any order. Q4_ERR_ARG and *out
 * untouched: an unknown kind or key, a key twice or missing, a malformed number, a value q4_set_rope_scaling refuses. (CUSTOM has no text form.) */
int q4_parse_rope_scaling(const char* text, q4_rope_scaling* out);
/* Host only, no GPU: the head_size/2 frequencies a model of this head size and theta gets under s, as defined above; s NULL or kind NONE gives the f_i
 * themselves (rounded to float). Q4_ERR_ARG: a scaling the setter refuses, an odd or non-positive head_size, a theta that is not finite and positive,
 * CUSTOM with n_freqs != head_size / 2. */
int q4_rope_inv_freq(const q4_rope_scaling* s, int head_size, float rope_theta, float* out);
int q4_get_rope_inv_freq(const Transformer* t, float* out);          /* head_size/2 floats; Q4_ERR_ARG for an unscaled model: it has no frequency array */
/* Op-level form of fusion level 0's rotation for a scaled model: q4_rope_rotation with the angle (float)*pPos * inv_freq_dev[i], inv_freq_dev
 * [head_size/2] floats on the device */
int q4_rope_rotation_freqs(q4_half* q, q4_half* k, int num_heads, int num_kv_heads, int head_size, const int* pPos, int loff,
                           const float* inv_freq_dev);
/* 1: at fusion levels 4 / 5 a layer's FFN half of these sizes runs as one launch on the current device and stream (csrc/gemv_ffn_pair.h) */
int q4_ffn_pair_covers(int dim, int hidden_dim);
/* 1 (default): hipGraph capture/replay as USE_CUDA_GRAPHS llama2_q4.cu:33; 0: eager launches with the exact context length (the
 * reference's other path, :374); 2: eager launches with the graph path's sequence-length bin -- exactly what the graphs run, one launch
 * at a time (the mode to profile in: rocprofv3 cannot trace inside a graph capture) */
void q4_set_use_graphs(int enable);
void q4_reset_graphs(void);   /* drop captured graphs (main() cleanup llama2_q4.cu:713-716) */
/* Graphs captured so far in this process. Captured graphs are kept per model (RunState), for up to four live models: a host that alternates
 * them replays each one's graphs; beyond four the least recently used model's graphs are dropped and captured again on its next turn --
 * this counter is how a host sees that happen. */
int q4_graph_captures(void);

/* Per-token log-probability records inside the decode step (opt-in, per model; off by default, and then every launch list, every captured graph and
 * every bit is what it is without this call). top_k = -1: off; 0: the chosen / target token's log-probability only; 1 .. Q4_MAX_TOP_LOGPROBS: also
 * that many top alternatives. Anything else, a top_k above the vocabulary, or a Transformer the library did not build: Q4_ERR_ARG. Allocates a device
 * ring of seq_len records {lse, token_logprob, top_ids[K], top_logprobs[K]} (freed by q4_free_transformer or by top_k = -1) and drops the model's
 * captured graphs that contain the launch; the next steps capture again. The records are those of q4_logprob_topk: the model's own distribution,
 * temperature 1, no nucleus.
 * Record p describes step p's logits and the token at ring index p + 1: on a prompt step (gen_token = 0) token_logprob is that of the prompt token
 * tokens[p + 1]; on a greedy generated step it is entry 0 of the top order (the greedy token, same bits as top_logprobs[0]); on a sampled step it is
 * that of the token the sampler chose, inside the top k or not. One extra launch per step in front of the sampler (two on sampled steps: a one-wave
 * launch behind the sampler looks the chosen token up), in every graph variant and in the eager modes. Steps queued past an EOS write records nobody
 * reads; that is harmless. */
int q4_set_logprobs(Transformer* t, int top_k);
int q4_get_logprobs_k(const Transformer* t);      /* -1: off, or a Transformer the library did not build */
/* Synchronises the stream (like the parity dumps), then copies records first_pos .. first_pos + n - 1 to the host: token_logprob [n], top_ids and
 * top_logprobs [n x K] (K = q4_get_logprobs_k). Any of the three may be NULL. Records off, or positions outside [0, seq_len]: Q4_ERR_ARG. */
int q4_get_logprobs(const Transformer* t, int first_pos, int n, float* token_logprob, int* top_ids, float* top_logprobs);
/* Records inside prompt passes and verify passes (below; DESIGN.md 3.7 / 3.8, "With records"). Per model, off by default: off, records on keep every
 * position on per-token steps, and the admission, every launch list, every captured graph, every bit and every counter are what they are without this
 * call. on != 0 lifts only that one exclusion; everything else a pass requires stays, and with records on a prompt pass also needs the verify pass's
 * classifier shape (dim 4096, a vocabulary that is a multiple of 8). A prompt pass then runs that classifier over its rows and the row form of the record
 * launch (q4_logprob_topk_rows; the target of a row is the next prompt token) and leaves its last row in RunState::logits, as the last prompt step would.
 * A verify pass runs the row form between its classifier and its accept launch (greedy: token_logprob is entry 0; under the sampler the raw rows are
 * kept aside and the chosen tokens looked up behind the sampler's row form). Records p .. p + m of a verify pass that accepts m drafts are what m + 1
 * steps write. Records p + m + 1 .. p + D describe rejected drafts: they lie at or above the device position and are rewritten by whatever runs there
 * next -- the same contract as the K / V rows of rejected drafts. q4_score_ids takes prompt passes with the switch on. Every record, token, K / V row and
 * the logits are those of the per-token run, byte for byte. Q4_ERR_ARG / 0: a Transformer the library did not build. */
int q4_set_pass_logprobs(Transformer* t, int on);
int q4_get_pass_logprobs(const Transformer* t);   /* 1: on; 0: off, or not a Transformer the library built */
/* Prompt and verify passes for the grouped-query 4096-wide shape (Mistral-7B, Llama-3-8B): per model, off by default -- a grouped-query model then runs
 * per-token steps everywhere, as before, and no decision, launch or counter changes. On, q4_set_prompt_ingest's passes, the verify passes of
 * q4_set_speculative (greedy and, where the vocabulary admits it, q4_set_speculative_sampled), passes with records (q4_set_pass_logprobs) and
 * q4_score_ids through passes also admit a model with: dim 4096 and 128-wide heads; n_heads = 4 * n_kv_heads (K / V rows dim / 4 wide); a hidden size
 * whose down projection the step runs as the two-part K split with three whole k-slots and a shared last slot of at most 32 units per part (hidden
 * 14336: 448 units, 224 = 3 x 64 + 32 per part) -- and only while q4_set_ksplit / q4_set_half_tail of the profiling build leave that form in force;
 * and everything a pass requires of a multi-head model (a rotation table, an fp16 K / V cache, an unmasked stream, fusion level >= 3, the position, bin,
 * record, guide, adaptive and context-shift rules of q4_set_prompt_ingest and q4_verify_tokens). Other ratios, other head sizes, the FP8 cache (unless q4_set_pass_kv8
 * admits it) and 13B (q4_set_pass_13b, below) stay on steps. A multi-head model behaves with the switch on exactly as with it off. K / V rows, tokens, logits, records and rng_state are the
 * per-token run's, byte for byte; q4_verify_covers, q4_verify_covers_sampled and q4_prompt_passes report the admissions. Q4_ERR_ARG / 0: a Transformer
 * the library did not build. */
int q4_set_pass_gqa(Transformer* t, int on);
int q4_get_pass_gqa(const Transformer* t);        /* 1: on; 0: off, or not a Transformer the library built */
/* The CLI's Q4_PASS_GQA: "1" on, "0" off; anything else Q4_ERR_ARG and *on untouched. */
int q4_parse_pass_gqa(const char* text, int* on);
/* Prompt and verify passes for a model with the FP8 (e4m3) K / V cache (q4_set_kv_format(Q4_KV_FP8); csrc/prompt_pass_kv8.h, DESIGN.md 3.7 "FP8
 * cache"): per model, off by default -- an FP8 model then runs per-token steps everywhere, as before, and no decision, launch or counter changes. On,
 * q4_set_prompt_ingest's passes, the verify passes of q4_set_speculative (greedy and q4_set_speculative_sampled), passes with records
 * (q4_set_pass_logprobs), with logit stages (q4_set_pass_stages) and q4_score_ids through passes also admit an FP8 model of a shape they admit with the
 * fp16 cache: Llama-2-7B's and, with q4_set_pass_gqa on, the grouped-query 4096-wide one (128-wide heads either way). A pass leaves its K / V rows as
 * fp16 in staging rows, one launch per layer quantises and appends them exactly as the step's attention launch appends its row, and attention then reads
 * every row from the byte caches. It is taken where every position of the pass runs the step's one-pass attention with a bin argument of at most 256, or
 * all of them ONE split-context form (bin arguments from 512 up under q4_set_pass_context; without graphs positions 256 .. 510 therefore stay on steps).
 * Tokens, the e4m3 bytes and row exponents of every row below the position, logits, records, rng_state and guide states are the per-token run's on the
 * same cache format, byte for byte; rows of rejected drafts lie at or above the position and are rewritten by what runs there next. A model with the
 * fp16 cache behaves with the switch on exactly as with it off. Q4_ERR_ARG / 0: a Transformer the library did not build. */
int q4_set_pass_kv8(Transformer* t, int on);
int q4_get_pass_kv8(const Transformer* t);        /* 1: on; 0: off, or not a Transformer the library built */
/* The CLI's Q4_PASS_KV8: "1" on, "0" off; anything else Q4_ERR_ARG and *on untouched. */
int q4_parse_pass_kv8(const char* text, int* on);
/* Prompt and verify passes for Llama-2-13B's shape (DESIGN.md 3.7 "13B"): per model, off by default -- a 5120-wide model then runs per-token steps
 * everywhere, as before, and no decision, launch or counter changes. On, q4_set_prompt_ingest's passes, the verify passes of q4_set_speculative (greedy
 * and q4_set_speculative_sampled), passes with records (q4_set_pass_logprobs), with logit stages (q4_set_pass_stages) and q4_score_ids through passes
 * also admit a model with: dim 5120 as 128-wide heads, multi-head (n_heads = n_kv_heads = 40); hidden 13824, whose down projection the step runs as
 * the two-part K split with three whole k-slots and a shared last slot per part (432 units, 216 = 3 x 64 + 24 per part); an fp16 K / V cache; the
 * step's K = 5120 launches on their shipped forms (two whole k-slots and the shared half slot: the profiling build's q4_set_half_tail(0),
 * q4_set_ksplit(0 | 4), ablations and any GEMV form but the product's keep the steps); and everything a pass requires of a 4096-wide model (a rotation
 * table, an unmasked stream, fusion level >= 3, the position, bin, record, guide, adaptive and context-shift rules of q4_set_prompt_ingest and
 * q4_verify_tokens). Grouped-query models of this width, the FP8 cache (also with q4_set_pass_kv8 on) and other hidden sizes stay on steps. A model of
 * another width behaves with the switch on exactly as with it off. K / V rows, tokens, logits, records and rng_state are the per-token run's, byte for
 * byte; q4_verify_covers, q4_verify_covers_sampled and q4_prompt_passes report the admissions. Q4_ERR_ARG / 0: a Transformer the library did not build. */
int q4_set_pass_13b(Transformer* t, int on);
int q4_get_pass_13b(const Transformer* t);        /* 1: on; 0: off, or not a Transformer the library built */
/* The CLI's Q4_PASS_13B: "1" on, "0" off; anything else Q4_ERR_ARG and *on untouched. */
int q4_parse_pass_13b(const char* text, int* on);
/* Passes while a logit stage is on (csrc/spec_verify.h, DESIGN.md 3.8 "Under the logit stages"): per model, off by default -- off, a guide, DRY, the
 * sampling controls or the adaptive truncation switch every verify pass off and a guide or the adaptive truncation every prompt pass, as before, and
 * nothing else changes. On: a verify pass is admitted with a guide, DRY and the sampling controls on -- greedy and, with q4_set_speculative_sampled, under
 * the sampler --: between the classifier and the sampler / accept launch each stage rewrites the pass's logit rows through its row form, row r at position
 * p + r reading its tokens from a device view of the ring plus the drafts (an unverified token still never enters the ring). It keeps refusing the adaptive
 * truncation (typical-p, top-n-sigma, Mirostat), any stage together with log-probability records, and everything it refused before. A prompt pass is
 * admitted with a guide or the adaptive truncation on and puts their state by position to NONE over its positions, as prompt steps do. The library's token
 * loops then draft the guide's forced tokens first (q4_guide_forced_run) and ask the model's drafter only where that run is empty. Tokens, K / V rows,
 * logits, rng_state and the guide's state ring below the position are the per-token run's, byte for byte; states of rejected drafts lie at or above the
 * position and are rewritten by what runs there next. Q4_ERR_ARG / 0: a Transformer the library did not build. */
int q4_set_pass_stages(Transformer* t, int on);
int q4_get_pass_stages(const Transformer* t);     /* 1: on; 0: off, or not a Transformer the library built */
/* The CLI's Q4_PASS_STAGES: "1" on, "0" off; anything else Q4_ERR_ARG and *on untouched. */
int q4_parse_pass_stages(const char* text, int* on);

/* The classifier of a greedy step without streaming every fp16 row of wcls (csrc/cls_screen.h): where the classifier runs as strips (dim 4096 or
 * 5120, at least 64 vocabulary rows per CU, an unmasked stream) q4_build_transformer derives a per-row-scaled int8 copy of wcls (vocab x dim bytes: 131 MB
 * at 7B, 164 MB at 13B; a failed allocation leaves the model without it, which is not an error). A screened step streams that copy, bounds every logit,
 * computes the exact fp16 logit of the rows that can still be the largest and takes the argmax of those: the token is the one the full classifier gives, bit
 * for bit and tie for tie. RunState::logits then holds the exact logits of the candidate rows and -inf elsewhere, so only steps whose logits nobody reads are
 * screened: greedy generating steps (temperature 0) queued by the library's own token loops (q4_generate, q4_generate_ids, q4_chat) with copyLogits off,
 * log-probability records off and fusion level >= 1 -- and never the last step a generation queues: after q4_generate* returns, RunState::logits holds the
 * final position's full logits as before (a generation that stops at EOS ends on whatever step was queued last). q4_run_transformer, _at, _steps and
 * q4_run_llama_network never screen. q4_set_greedy_screen: 1 (default) on, 0 off; drops captured graphs like q4_set_fusion. */
void q4_set_greedy_screen(int on);
int q4_get_greedy_screen(void);
/* Candidate rows of the model's screened steps so far (synchronises the stream): of the last one, the largest, their sum, and the number of screened steps.
 * Any pointer may be NULL. All zero for a model without a screening copy; Q4_ERR_ARG for a Transformer the library did not build. */
int q4_screen_candidates(const Transformer* t, int* last, int* max, long long* total, long long* steps);

/* Prompt ingest (csrc/prompt_pass.h): the library's token loop (q4_generate, q4_generate_ids, q4_generate_ids_from) runs up to max_tokens
 * consecutive prompt-only positions -- those in front of num_prompt_tokens - 1, the step that generates -- as ONE pass over the weights: every launch reads
 * its weights once and multiplies all the positions' activations. The K / V rows, the generated tokens and the final logits are the per-token steps', bit
 * for bit; a pass runs no classifier, so RunState::logits is not written by the positions it covers. Taken only where the result is the same and nothing
 * reads what a pass leaves out: Llama-2-7B's geometry (dim 4096, multi-head, 128-wide heads, a hidden size the three-phase FFN launch admits; with
 * q4_set_pass_gqa on also the grouped-query shape described there, with q4_set_pass_13b on also Llama-2-13B's), fusion level
 * >= 3, an fp16 K / V cache (the FP8 cache with q4_set_pass_kv8 on), positions below the bound of q4_set_pass_context (256 unless raised), log-probability records off or q4_set_pass_logprobs on, no guide, no adaptive truncation, no context-shift offset, an unmasked
 * stream; everything else -- and q4_run_transformer*, q4_score_ids (unless q4_set_pass_logprobs is on), q4_perplexity_ids, q4_chat -- runs per token as before. max_tokens: 0 (or 1) off,
 * clamped to 8, the default. q4_prompt_passes: passes run since the library was loaded. */
void q4_set_prompt_ingest(int max_tokens);
int q4_get_prompt_ingest(void);
int q4_prompt_passes(void);
/* The exclusive upper bound on the positions a prompt pass or a verify pass (below) may touch. Process-wide, like q4_set_prompt_ingest; for a model the
 * bound in force is min(positions, seq_len). The default, 256, is also the least: arguments <= 256 give 256, and passes then stay in the bins where
 * the step's attention is the V-slice form, exactly as before the setting existed. A larger value lets passes follow the step into the split-context
 * bins (512, 1024, 2048, ...): there a pass's attention is one launch that reads each chunk of K / V rows once for all its tokens plus one that merges
 * every token's flash-decode records the way the step does -- the same bits, no in-launch wait. A pass never reaches across the end of a bin (256, 512,
 * 1024, ...), and is taken only where the step's attention form at every position it touches is one the pass reproduces (a model whose scratch does not
 * hold the records, or a residency guard that says no, keeps its steps). */
void q4_set_pass_context(int positions);
int q4_get_pass_context(void);
/* Op-level form of a screened step for tests and tools: x [n], w [d][n] and rms_w [n] (may be NULL: x is taken as it is) are device pointers to halves; a
 * screening copy of w is built and freed inside the call. Host outputs, any may be NULL: the greedy token, A and B [d] floats (approximate logit and radius,
 * B = +inf where no claim is made), the refined logits [d] halves (exact on candidate rows, -inf elsewhere), the number of candidate rows. Shapes the
 * classifier's strips do not cover: Q4_ERR_UNSUPPORTED_SIZE. */
int q4_greedy_screen_op(const q4_half* x, const q4_half* w, int n, int d, const q4_half* rms_w, int* token, float* A, float* B, q4_half* refined,
                        int* candidates);

/* ---- speculative greedy decoding (csrc/spec_verify.h). Not in the reference. Off by default. ----
 * A verify pass runs the token at the current position p and D drafted tokens (1 <= D <= Q4_SPEC_MAX_DRAFT) as the positions p .. p + D of ONE pass over the
 * weights, classifier included, and accepts the m leading drafts that equal the greedy token of the row in front of them. Every row's logits are the per-token
 * step's, bit for bit, so a pass emits exactly the m + 1 tokens that m + 1 greedy steps emit and leaves what they leave: ring[p + 1 .. p + m + 1], the
 * position p + m + 1, RunState::logits and RunState::x of step p + m, the K / V rows. K / V rows p + m + 1 .. p + D hold rows computed from rejected drafts:
 * they lie at or above the position (q4_common_prefix, q4_resume_sequence and snapshots never trust such rows) and are written again by whatever runs there next.
 * A pass is admitted where a prompt pass is (q4_set_prompt_ingest above: geometry, fusion level >= 3, fp16 cache, unmasked stream, no context-shift offset,
 * log-probability records off or q4_set_pass_logprobs on, no guide) and, in a token loop, only for a greedy sampler (temperature 0; q4_set_speculative_sampled below adds the
 * temperature / top-p sampler) with no logit stage on (sampling controls, logit bias, DRY, adaptive truncation), with p .. p + D inside one bin (ends at 256, 512, 1024, ...), below the bound of q4_set_pass_context
 * (256 unless raised), inside `steps` and seq_len. Cost (7B, measured: DESIGN.md 3.8): a pass pays where drafts are usually
 * right and loses where they are not. */
#define Q4_SPEC_MAX_DRAFT 7
#define Q4_SPEC_MAX_NGRAM 8
/* The primitive, at the current position (synchronises before and after): out_tokens receives the *n_accepted + 1 tokens the pass emitted (room for
 * n_draft + 1), the first *n_accepted of them equal to draft[]. Q4_ERR_ARG before any launch: a null pointer, n_draft outside 1 .. Q4_SPEC_MAX_DRAFT, an id
 * outside [0, vocab), a Transformer the library did not build. Q4_NOT_ADMITTED, nothing done: the model, the settings or the position do not admit a pass
 * (q4_verify_covers). The caller owns the sequence (q4_reset_sequence, then steps or passes); greedy, whatever a Sampler says.
 * Logit stages: the greedy primitive has no Sampler, so of the stages it knows the model's guide alone -- admitted with q4_set_pass_stages on, and the rows
 * are then masked as the guided greedy step masks them. DRY and the sampling controls live beside a Sampler: a host that wants them inside a pass hands
 * that Sampler to q4_verify_tokens_sampled (temperature above 0) or runs the library's token loop, whose greedy passes take the stages of the loop's Sampler. */
int q4_verify_tokens(Transformer* t, const int* draft, int n_draft, int* out_tokens, int* n_accepted);
int q4_verify_covers(const Transformer* t, int pos, int n_draft);      /* 1: q4_verify_tokens at position pos with n_draft drafts would run; else 0 */
/* The library's token loops (q4_generate, q4_generate_ids, q4_generate_ids_from): at a generating position whose pass is admitted the loop asks the model's
 * drafter for up to max_draft tokens behind the ring and, when it gets any, runs one verify pass instead of steps; else it queues steps as before and asks
 * again behind them. Tokens, K / V rows, final logits and the Sampler's random stream are those of the loop without it. max_draft 0: off (the default,
 * ngram_* ignored); else 1 <= max_draft <= Q4_SPEC_MAX_DRAFT and 1 <= ngram_min <= ngram_max <= Q4_SPEC_MAX_NGRAM (the built-in drafter's), or Q4_ERR_ARG. */
int q4_set_speculative(Transformer* t, int max_draft, int ngram_max, int ngram_min);
int q4_get_speculative(const Transformer* t, int* max_draft, int* ngram_max, int* ngram_min);
/* "draft=4,ngram=3,min=2": any subset of the keys in any order; a key left out takes draft=4, ngram=3, min=2 (min: the value of ngram where that is 1; DESIGN.md 3.8
 * has the measurements behind them); "draft=0" is off. Q4_ERR_ARG and the outputs
 * untouched: an unknown key, a malformed number, a trailing comma, values q4_set_speculative refuses. */
int q4_parse_speculative(const char* text, int* max_draft, int* ngram_max, int* ngram_min);
/* A drafter: tokens[0 .. n_tokens) is the ring up to the current position's token; it writes up to max_draft ids to draft_out and returns how many (<= 0:
 * none; ids outside the vocabulary end the draft in front of them). Called on the host from inside the token loop. NULL: the built-in drafter. */
typedef int (*q4_drafter_fn)(void* ctx, const int* tokens, int n_tokens, int max_draft, int* draft_out);
int q4_set_drafter(Transformer* t, q4_drafter_fn fn, void* ctx);
/* The built-in (prompt-lookup) drafter, host only: for g = ngram_max down to ngram_min (g < n_tokens), the most recent EARLIER occurrence of the last g
 * tokens -- tokens[j .. j + g) == tokens[n_tokens - g .. n_tokens) with j < n_tokens - g, the largest such j -- and what followed it: tokens[j + g ..), up to
 * max_draft of them and no further than the ring's end. The first g with a match decides. Returns the number of ids written, 0 for no match or bad
 * arguments. */
int q4_spec_draft(const int* tokens, int n_tokens, int max_draft, int ngram_max, int ngram_min, int* draft_out);
/* Verify passes run with this model, the drafts they carried and the drafts accepted, since the model was built. Any pointer may be NULL. */
int q4_spec_stats(const Transformer* t, long long* passes, long long* drafted, long long* accepted);
/* Of those drafts, the ones the guide's forced run gave the token loop (q4_set_pass_stages) and how many of them were accepted. Any pointer may be NULL. */
int q4_spec_stats_forced(const Transformer* t, long long* drafted, long long* accepted);
/* Op-level forms of the pass's two launches for tests and tools, on the q4 stream; device pointers unless said otherwise.
 * q4_verify_classifier: logits [n_rows][vocab] = wcls . rmsnorm(x[r], rms_w), x [n_rows][dim], 1 <= n_rows <= 8; every row holds the bits q4_rmsnorm +
 * q4_matmul_f16 give for that row alone. dim 4096 and a vocabulary that is a multiple of 8, else Q4_ERR_UNSUPPORTED_SIZE.
 * q4_verify_accept: logits rows of `size` halves, `ld` halves apart (ld a multiple of 8, >= size), row r the logits at position *pos_dev + r, r <= n_draft;
 * draft: host array. Takes each row's greedy token by q4_argmax's rule, m = the leading rows r < n_draft whose token equals draft[r], and writes
 * ring[p + 1 .. p + m + 1], logits_out [size] = row m, x_out [dim] = row m of x [n_draft + 1][dim] (x may be NULL: no copy), then *pos_host and *pos_dev =
 * p + m + 1. report (9 ints, may be NULL): the rows' tokens (-1 past row n_draft) and m. */
int q4_verify_classifier(q4_half* logits, const q4_half* x, const q4_half* rms_w, const q4_half* wcls, int dim, int vocab, int n_rows);
int q4_verify_accept(const q4_half* logits, int ld, int size, const int* draft, int n_draft, const q4_half* x, int dim, q4_half* logits_out, q4_half* x_out,
                     int* ring, int* pos_host, int* pos_dev, int* report);

/* ---- verify passes under the temperature / top-p sampler ("Under the sampler"). Off by default; a switch of its own. ----
 * A sampled step is a function of its logits and one coin, and the coin is a function of (seed, position). With the switch on, a pass under a sampler with
 * a finite temperature above 0 samples EVERY row with its own position's coin -- the step's two sampler launches, one grid slice per row, each row
 * normalised in place -- and accepts the leading drafts that equal the sampled tokens. Lossless: tokens, K / V rows, RunState::logits (row m's fp16
 * probabilities, what the sampled step leaves there) and the Sampler's random state are those of the run without it, byte for byte. On top of the greedy
 * admission: no logit stage on, a vocabulary of at most 32768 entries (a multiple of 8); a negative temperature, a larger vocabulary or the switch off
 * run steps. A drafter's tokens are point guesses: the chance that a draft is accepted is the target's probability of it. Rejection sampling against a
 * sampling draft model (min(1, p / q)) is not this and not here. */
int q4_set_speculative_sampled(Transformer* t, int on);
int q4_get_speculative_sampled(const Transformer* t);                  /* 1: on; 0: off, or not a Transformer the library built */
/* The CLI's Q4_SPECULATIVE_SAMPLED (a variable of its own beside Q4_SPECULATIVE): "1" on, "0" off; anything else Q4_ERR_ARG and *on untouched. */
int q4_parse_speculative_sampled(const char* text, int* on);
/* q4_verify_tokens under `sampler`: same contract (Q4_ERR_ARG before any launch, a null sampler included; Q4_NOT_ADMITTED when nothing ran, the switch off
 * or temperature 0 included). The sampler's stream must stand at the current position's coin; the call consumes *n_accepted + 1 coins of it, one per
 * position that ran, as that many steps would. */
int q4_verify_tokens_sampled(Transformer* t, Sampler* sampler, const int* draft, int n_draft, int* out_tokens, int* n_accepted);
int q4_verify_covers_sampled(const Transformer* t, const Sampler* sampler, int pos, int n_draft);   /* 1: q4_verify_tokens_sampled would run there; else 0 */
/* Op-level forms, for tests and tools, on the q4 stream.
 * q4_verify_sample_rows: rows r < n_rows (1 .. 8) of logits (device, `ld` halves apart, ld a multiple of 8 and >= the sampler's vocabulary) are normalised IN
 * PLACE and sampled with coins_host[r] (host array) under the sampler's temperature / top-p: tokens_dev[r] (device) and the row's probabilities are what
 * q4_sample leaves for that row alone with that coin. Nothing else is written; halves behind a row's vocabulary are neither read nor written.
 * Q4_ERR_UNSUPPORTED_SIZE: a vocabulary above 32768 or no multiple of 8, a temperature that is not finite and above 0.
 * q4_verify_accept_tokens: q4_verify_accept with the rows' tokens given in tokens_dev (device, n_draft + 1 ints) instead of each row's argmax. */
int q4_verify_sample_rows(Sampler* sampler, q4_half* logits, int ld, int n_rows, const float* coins_host, int* tokens_dev);
int q4_verify_accept_tokens(const q4_half* logits, int ld, int size, const int* draft, int n_draft, const int* tokens_dev, const q4_half* x, int dim,
                            q4_half* logits_out, q4_half* x_out, int* ring, int* pos_host, int* pos_dev, int* report);

/* build_sampler / destroy_sampler sampler.h:15-29; random_u32 / random_f32 :31-40; sample :43-82 */
int build_sampler(Sampler* sampler, int vocab_size, float temperature, float topp, unsigned long long rng_seed);
void destroy_sampler(Sampler* sampler);
unsigned int random_u32(unsigned long long* state);
float random_f32(unsigned long long* state);
int q4_sample(Sampler* sampler, RunState* s, int gen_token);

/* Not in the reference: the sampling controls of a completion API beside temperature and top-p -- top-k, min-p, repetition / presence / frequency
 * penalties, a logit bias -- applied on the device inside the decode step (csrc/q4_logit_process.hip), so that a host which wants them keeps the
 * multi-step graphs and the queued-ahead step. The Sampler struct keeps the reference's layout: the controls live beside it, keyed by its address;
 * destroy_sampler / q4_sampler_delete free them. Off by default, and then every launch list, every captured graph and every bit is what it is without
 * these calls.
 * With controls on, every GENERATING step (gen_token != 0) that uses the sampler -- greedy or sampled, eager or in any graph variant, one or
 * Q4_MULTI_STEPS per replay -- runs one one-block launch behind the log-probability record launch and in front of the argmax / sampler. It rewrites
 * RunState::logits in place; for token i with half logit l, v = float(l), every operation one IEEE fp32 operation:
 *   1. bias: i in the bias list: v = v + b_i.
 *   2. penalties: W = the ring entries tokens[max(0, pos + 1 - penalty_last_n) .. pos], pos the step's position (prompt tokens count; entries outside
 *      the vocabulary do not), read only while a penalty is not neutral; c_i = occurrences of i in W. c_i > 0: v = v > 0 ? v / repeat_penalty :
 *      v * repeat_penalty, then v = v - (float(c_i) * frequency_penalty + presence_penalty). The window is read from the ring by position in every step:
 *      q4_reset_sequence, rewinds and q4_run_transformer_at need no bookkeeping.
 *   3. a finite v is clamped to +-65504 and rounded to half (nearest even); an infinity stays; a NaN result is the quiet NaN 0x7E00. Only the entries
 *      touched by 1 and 2 are rewritten.
 *   4. top_k (0: off): in the order (value descending, index ascending) -- -0 equals +0, a NaN ranks last, ties across rank k are resolved by index --
 *      the first top_k entries stay, every other becomes -inf.
 *   5. min_p (0: off): with m the largest processed logit, entry i stays iff float(l_i) - float(m) >= logf(min_p), else it becomes -inf. This is min-p
 *      on the PROCESSED logits AT TEMPERATURE 1: it does not depend on the sampler's temperature.
 * Log-probability records and copyLogits are taken in front of the launch: they keep describing the model's own raw distribution (the token_logprob
 * of a greedy step is then that of the token the step chose, which need not be entry 0 of the raw order: it is looked up behind the argmax, as on a
 * sampled step). After a greedy
 * generating step RunState::logits holds the PROCESSED logits (after a sampled one the sampler's probabilities, as always). Prompt steps launch nothing.
 * Greedy steps are not screened (q4_set_greedy_screen) while controls are on. q4_sample itself is unchanged: a host with its own per-step loop calls
 * q4_process_logits in front of it.
 * The values may change between steps: the next step sees them, no captured graph is replayed with stale ones (graphs are captured again only when the
 * controls go from off to on or back). */
enum { Q4_MAX_PENALTY_WINDOW = 1024, Q4_MAX_LOGIT_BIAS = 256 };
typedef struct {
    int top_k;                 /* 0: off */
    float min_p;               /* [0, 1), 0: off */
    float repeat_penalty;      /* > 0, 1: off */
    float presence_penalty;    /* 0: off */
    float frequency_penalty;   /* 0: off */
    int penalty_last_n;        /* [0, Q4_MAX_PENALTY_WINDOW] */
} q4_sampling_controls;
/* NULL or all-neutral {0, 0, 1, 0, 0, any}: off. Q4_ERR_ARG (nothing changes, the GPU is not touched): top_k < 0, min_p outside [0, 1), repeat_penalty
 * <= 0 or not finite, a presence or frequency penalty that is not finite, penalty_last_n outside [0, Q4_MAX_PENALTY_WINDOW]. A top_k or a bias id beyond
 * the vocabulary is found by the first step that uses the sampler with a model: that step returns Q4_ERR_ARG. */
int q4_sampler_set_controls(Sampler* sampler, const q4_sampling_controls* controls);
int q4_sampler_get_controls(const Sampler* sampler, q4_sampling_controls* out);
/* ids / bias: host arrays of n <= Q4_MAX_LOGIT_BIAS entries, copied; n = 0 clears. Q4_ERR_ARG: an id that is negative or listed twice, a bias that is NaN,
 * +inf or above 65504 in magnitude (-inf is allowed: it bans the token). */
int q4_sampler_set_logit_bias(Sampler* sampler, const int* ids, const float* bias, int n);
/* "top_k=40,min_p=0.05,repeat_penalty=1.1,last_n=64,presence=0,frequency=0": any subset of the keys in any order; a key left out keeps its neutral
 * value (last_n: 64). Q4_ERR_ARG and *out untouched: an unknown key, a malformed number, a value q4_sampler_set_controls refuses. */
int q4_parse_sampling_controls(const char* text, q4_sampling_controls* out);
/* Op-level form of the launch: logits [n] halves (16-byte aligned), tokens (the ring) and pPos (one int: the position) device-visible -- both may be
 * NULL: no window --, bias_ids / bias host arrays. Rewrites logits in place on the q4 stream. top_k > n, a bias id >= n or anything the setters refuse:
 * Q4_ERR_ARG without touching the GPU. */
int q4_process_logits(q4_half* logits, int n, const q4_sampling_controls* controls, const int* bias_ids, const float* bias, int n_bias,
                      const int* tokens, const int* pPos);
/* The row form (a verify pass with q4_set_pass_stages on): rows r < n_rows of logits, `ld` halves apart, row r rewritten at position pos_rows_dev[r] with
 * its window read from tokens_view_dev (device, tokens by absolute position) -- byte for byte what q4_process_logits writes for that row alone at that
 * position; halves between n and ld are neither read nor written. Also Q4_ERR_ARG: n_rows outside 1 .. 8, ld < n, ld not a multiple of 8. */
int q4_process_logits_rows(q4_half* logits, int n, const q4_sampling_controls* controls, const int* bias_ids, const float* bias, int n_bias, int ld,
                           int n_rows, const int* tokens_view_dev, const int* pos_rows_dev);

/* ---- DRY and no-repeat-n-gram penalties (q4_dry.hip; not in the reference) ----------------------
 * The two controls of a completion API against loops: DRY ("don't repeat yourself") penalises only the token that would extend a repeated sequence, the
 * more the longer the match; no_repeat_ngram_size is the hard ban of the same family. Both match the sequence's suffix against its own history, on the
 * device inside the decode step: with either on, every GENERATING step that uses the sampler -- greedy or sampled, eager or in any graph variant -- runs
 * one one-block launch BEHIND the guide's launch and IN FRONT OF the sampling controls' launch (a guide's -inf stays -inf; top-k and min-p count what
 * DRY left). Kept beside the Sampler, keyed by its address, like the sampling controls; off by default, and then every launch list, every captured
 * graph and every bit is what it is without these calls. The rule reads the ring in every launch and keeps no state: nothing has to be reset, rewound
 * or moved (resume, roll-back, snapshots and context shift need no bookkeeping).
 *   ring = the token ring (SharedData::tokens; entries compare as plain ints), p = the step's position (*pPos before the sampler advances it),
 *   W = ring indices [start, p], start = max(0, p + 1 - last_n) (prompt tokens count), CAP = Q4_DRY_MAX_MATCH.
 *   R   = the number of consecutive non-breaker entries going back from ring[p] (ring[p], ring[p-1], ...), counted inside W, capped at CAP; a breaker at
 *         ring[p] gives R = 0.
 *   M_i, for every i in [start, p) with ring[i] == ring[p]: the largest M in [1, CAP] with ring[i-j] == ring[p-j] for all 0 <= j < M and
 *         i - (M-1) >= start (the two ranges may overlap: periodic sequences are the main case).
 *   t = ring[i+1] is the token that would extend the repetition; a t outside [0, n) is ignored. Per distinct t: M_t = max_i M_i, L_t = min(M_t, R).
 * Per touched t, v = float(logits[t]):
 *   ban: no_repeat_ngram_size = N >= 2 and M_t >= N - 1: the logit becomes -inf (0xFC00). The ban ignores breakers.
 *   DRY: otherwise, multiplier > 0 and L_t >= allowed_length: v = v - pen[L_t], ONE IEEE fp32 subtraction, finished as step 3 of the sampling
 *        controls: a finite value clamped to +-65504 and rounded to half (nearest even), an infinity stays, a NaN becomes 0x7E00.
 * pen[L], L = 0 .. 64, is computed on the host (q4_dry_penalty_table): multiplier * powf(base, L - allowed_length) clamped to 3.0e38 for
 * L >= allowed_length, 0 below; it travels in the parameter block, the kernel calls no transcendental. Every other logit keeps its 16 bits. No float
 * atomics, no arrival order: the same input gives the same bytes on every launch. No ring entry or breaker id indexes anything before it has been
 * checked against [0, n).
 * Log-probability records and copyLogits are taken in front of the launch and describe the raw distribution (a greedy step's token_logprob is looked up
 * behind the argmax); after a greedy generating step RunState::logits holds the processed logits; greedy steps are not screened while DRY is on; prompt
 * steps launch nothing. Values and breakers may change between steps without a new capture (graphs hold the address of a small device block only). */
enum { Q4_MAX_DRY_WINDOW = 4096, Q4_DRY_MAX_MATCH = 64 };
typedef struct {
    float multiplier;          /* >= 0, finite; 0: no DRY penalty */
    float base;                /* >= 1, finite */
    int allowed_length;        /* [1, Q4_DRY_MAX_MATCH] */
    int last_n;                /* [0, Q4_MAX_DRY_WINDOW] */
    int no_repeat_ngram_size;  /* 0: off, else [2, Q4_DRY_MAX_MATCH + 1] */
} q4_dry_controls;
/* NULL: off (the defaults {0, 1.75, 2, 1024, 0} come back). Off also: multiplier == 0 && no_repeat_ngram_size == 0, or last_n == 0. A value outside the
 * ranges above: Q4_ERR_ARG, nothing changes, the GPU is not touched. */
int q4_sampler_set_dry(Sampler* sampler, const q4_dry_controls* controls);
int q4_sampler_get_dry(const Sampler* sampler, q4_dry_controls* out);
/* Sequence breakers: single tokens a match does not reach across. ids: a host array of any number of distinct ids >= 0, copied; n = 0 clears. The step
 * turns them into a vocabulary bitmap on the device. Q4_ERR_ARG: a negative or repeated id. An id at or above the vocabulary is found by the first step
 * that uses the sampler with a model: that step returns Q4_ERR_ARG. */
int q4_sampler_set_dry_breakers(Sampler* sampler, const int* ids, int n);
/* "multiplier=0.8,base=1.75,allowed=2,last_n=1024,ngram=0": any subset of the keys in any order; a key left out keeps that value (multiplier: 0).
 * Q4_ERR_ARG and *out untouched: an unknown key, a malformed number, a trailing comma, a value q4_sampler_set_dry refuses. */
int q4_parse_dry(const char* text, q4_dry_controls* out);
/* Host only: pen[0 .. 64] as above. Q4_ERR_ARG for controls the setter refuses. */
int q4_dry_penalty_table(const q4_dry_controls* controls, float out[65]);
/* Op-level form of the launch on the q4 stream: logits [n] halves, tokens (the ring, at least *pPos + 1 entries) and pPos (one int) device-visible --
 * both may be NULL: no window --, breaker_ids a host array. Anything the setters refuse, or a breaker id >= n: Q4_ERR_ARG without touching the GPU. */
int q4_dry_penalty(q4_half* logits, int n, const q4_dry_controls* controls, const int* breaker_ids, int n_breakers, const int* tokens,
                   const int* pPos);
/* The row form (a verify pass with q4_set_pass_stages on): rows r < n_rows of logits, `ld` halves apart, row r rewritten at position pos_rows_dev[r] with
 * its window read from tokens_view_dev (device, tokens by absolute position) -- byte for byte what q4_dry_penalty writes for that row alone at that
 * position; halves between n and ld are neither read nor written. Also Q4_ERR_ARG: n_rows outside 1 .. 8, ld < n, ld not a multiple of 8. */
int q4_dry_penalty_rows(q4_half* logits, int n, const q4_dry_controls* controls, const int* breaker_ids, int n_breakers, int ld, int n_rows,
                        const int* tokens_view_dev, const int* pos_rows_dev);

/* ---- typical-p, top-n-sigma and Mirostat v2 (q4_adaptive.hip; not in the reference) -------------
 * Three truncation rules of completion APIs that take their threshold from a statistic of the whole distribution. With one of them on, every GENERATING
 * step that uses the sampler -- greedy or sampled, eager or in any graph variant -- runs one one-block launch BEHIND the sampling controls' launch and IN
 * FRONT OF the argmax / sampler (order in the step: guide, DRY, controls, this; typical-p and Mirostat see what top-k and min-p left; a -inf stays -inf).
 * Kept beside the Sampler, keyed by its address; off by default, and then every launch list, every captured graph and every bit is what it is without
 * these calls. Values may change between steps without a new capture (graphs hold the address of a small device block only); going from off to on or
 * back captures again. Log-probability records and copyLogits are taken in front and describe the raw distribution (a greedy step's token_logprob is
 * looked up behind the argmax); greedy steps are not screened while it is on; prompt steps launch nothing.
 *   v_i = float(l_i) of the half logits as the launch finds them. An entry TAKES PART iff it is finite; -inf, +inf and NaN entries are left as they are
 *   and enter no statistic. A masked entry becomes 0xFC00 (-inf) and takes no part in the stages behind; every other entry keeps its 16 bits.
 *   Every statistic is an fp32 sum in one fixed order (q4_logprobs.hip's: per thread runs of 32 in ascending index, the runs' totals, the tail element; a
 *   64-lane tree; a 16-lane tree) -- the same bytes on every launch. Each operation below is ONE IEEE fp32 operation (no contraction).
 * 1. top-n-sigma (top_n_sigma > 0): m = the largest v_i, mean = (sum v_i) / count, sigma = sqrtf((sum (v_i - mean)^2) / count),
 *    T_s = m - top_n_sigma * sigma; entry i stays iff v_i >= T_s.
 * 2. typical-p (typical_p < 1), on what 1 left, at temperature 1: lse = m + logf(sum expf(v_i - m)); s_i = lse - v_i; p_i = expf(-s_i);
 *    H = sum p_i * s_i; d_i = fabsf(s_i - H). Entry i stays iff d_i <= d*, d* the smallest d_i occurring for which the fp32 sum (that order) of the p_i
 *    with d_i <= d* is >= typical_p -- a whole tier of equal d_i stays or goes together; where even the whole sum stays below typical_p, everything stays.
 * 3. Mirostat v2 (mirostat_tau > 0), on what 1 and 2 left, at the SAMPLER's temperature t (temperature 0: the step returns Q4_ERR_ARG). State: a ring
 *    mu[seq_len] of float per model, by position (none: a NaN, every byte 0xFF), and a side buffer of vocab floats + {side_pos, side_lse}, both allocated
 *    by the first step that needs them. At position p (*pPos before the sampler advances it): prev = mu[p - 1], none at p = 0.
 *      prev none: mu_p = 2 * tau (a span starts);
 *      else if side_pos == p - 1 and tok = tokens[p] is in [0, n) with a finite side[tok]:
 *           surprise = (side_lse - side[tok]) * 1.44269504f; mu_p = prev - eta * (surprise - tau);
 *      else mu_p = prev (a rewind with q4_run_transformer_at).
 *    w_i = v_i / t; lse_t = w_max + logf(sum expf(w_i - w_max)); T_m = lse_t - mu_p * 0.693147181f; entry i stays iff w_i >= T_m; the entry of largest w
 *    (lowest index on ties) always stays. Then mu[p] = mu_p; side[i] = w_i of the entries that stayed, -inf elsewhere; side_lse = their log-sum-exp;
 *    side_pos = p. For Mirostat as published run with topp = 1: a top-p below 1 truncates further behind it.
 * Prompt groups run with a sampler that has the launch on write none over their positions (with it off a prompt step launches and clears nothing, as
 * before this feature); q4_reset_sequence and q4_resume_sequence write none over the ring (every resume passes a prompt step, so a
 * span restarts behind it). q4_shift_context moves ring entries and records with the rows, entry n_pos - n_discard - 1 receives old entry n_pos - 1, and
 * side_pos is rebased. Snapshots carry nothing of it. A RunState the library did not build has no rings: Mirostat is Q4_ERR_ARG there. */
enum { Q4_ADAPTIVE_RECORD = 8 };
typedef struct {
    float typical_p;       /* (0, 1]; 1: off */
    float top_n_sigma;     /* >= 0, finite; 0: off */
    float mirostat_tau;    /* >= 0, finite; 0: Mirostat off */
    float mirostat_eta;    /* (0, 1] */
} q4_adaptive_controls;
/* NULL: off (the neutral values {1, 0, 0, 0.1} come back). All of typical_p == 1, top_n_sigma == 0, mirostat_tau == 0: off. A value outside the ranges
 * above (a NaN is outside every range): Q4_ERR_ARG, nothing changes, the GPU is not touched. */
int q4_sampler_set_adaptive(Sampler* sampler, const q4_adaptive_controls* controls);
int q4_sampler_get_adaptive(const Sampler* sampler, q4_adaptive_controls* out);
/* "typical_p=0.9,top_n_sigma=1.5,mirostat_tau=5,mirostat_eta=0.1": any subset of the keys in any order, each at most once; a key left out keeps its
 * neutral value. Q4_ERR_ARG and *out untouched: an unknown key, a key given twice, a malformed number, a trailing comma, a value the setter refuses. */
int q4_parse_adaptive(const char* text, q4_adaptive_controls* out);
/* The records of the launches at positions [first_pos, first_pos + n): Q4_ADAPTIVE_RECORD floats each, {T_s, H, d*, mu, T_m, kept, lse, lse_t} -- kept is
 * the number of finite entries behind the launch as the BITS of an int; a NaN where a stage was off or no launch ran. (lse and lse_t are recorded so
 * that the masks can be recomputed exactly from the record.) Synchronises. Q4_ERR_ARG: no launch has run with this model yet, a range outside the ring. */
int q4_get_adaptive_records(const Transformer* t, int first_pos, int n, float* out);
/* Op-level form of the launch on the q4 stream: logits [n] halves in place. With Mirostat on: temperature > 0, mu_ring (at least *pPos + 1 floats), side
 * (n + 2 floats; side_pos is an int), tokens (the ring) and pPos (one int) device-visible; with Mirostat off all four may be NULL and the position is
 * not read. record: Q4_ADAPTIVE_RECORD floats on the device, or NULL. Q4_ERR_ARG without touching the GPU: anything the setter refuses, Mirostat with a
 * temperature that is not above 0 or a missing pointer. */
int q4_adaptive_mask(q4_half* logits, int n, const q4_adaptive_controls* controls, float temperature, float* mu_ring, float* side, const int* tokens,
                     const int* pPos, float* record);

/* ---- guided decoding (q4_guide.hip; not in the reference) --------------------------------------
 * A constraint over tokens as a finite automaton: S states (state 0 starts), a dense table next[s][i] of uint16_t, each entry a state in [0, S) or
 * Q4_GUIDE_DEAD (state s forbids token i). A guide is immutable and lives on the device: S rows of the vocabulary rounded up to 8 entries, 2 * S * V
 * bytes (64 KB per state at 32000 tokens). A model with a guide attached keeps the automaton's state on the device, by position, in a ring
 * state[seq_len] of int: Q4_GUIDE_NONE where no guided step ran, Q4_GUIDE_OFFTRACK (sticky) once a token the guide forbids was consumed. Every
 * GENERATING step of such a model carries one one-block launch between the record launch and the sampling controls' launch (or the argmax / sampler):
 * with p the step's position,
 *   prev = p > 0 ? state[p - 1] : NONE;
 *   s = 0 if prev == NONE; OFFTRACK if prev == OFFTRACK or prev is outside [0, S); else with t = tokens[p] (the pinned ring):
 *       next[prev][t] if 0 <= t < V and that entry is not DEAD, else OFFTRACK;
 *   state[p] = s; unless s == OFFTRACK, every logit i with next[s][i] == DEAD becomes -inf (0xFC00); every other logit keeps its 16 bits.
 * A position outside [0, seq_len) does nothing. Nothing returns to the host between steps: the multi-step replays, the queued-ahead step and the in-graph
 * sampler stay. A prompt step writes NONE at its position, q4_reset_sequence and q4_set_guide write NONE everywhere: a guided span begins at the first
 * generating step behind a prompt step (or at position 0), a rewind with q4_run_transformer_at inside a span continues from state[p - 1], a chat's next
 * turn starts at state 0 again. Log-probability records and copyLogits are taken in front of the launch and describe the raw distribution (a greedy
 * step's token_logprob is then looked up behind the argmax); after a greedy generating step RunState::logits holds the masked logits; greedy steps are
 * not screened while a guide is attached. Without a guide: the same launches, graphs and bits as before, nothing allocated. */
enum { Q4_GUIDE_MAX_STATES = 4096, Q4_GUIDE_DEAD = 0xFFFF, Q4_GUIDE_NONE = -1, Q4_GUIDE_OFFTRACK = -2 };
typedef struct q4_guide q4_guide;                       /* opaque, device-resident, immutable; may be attached to several models of the same vocabulary */
/* next: host, [n_states][vocab_size]. Q4_ERR_ARG without touching the GPU: n_states outside [1, Q4_GUIDE_MAX_STATES], vocab_size < 1, an entry that is
 * neither a state nor DEAD, a state without a live entry (the generated sequence could never leave it). Q4_ERR_ALLOC: no device memory for the table. */
int q4_guide_new(q4_guide** out, int n_states, int vocab_size, const uint16_t* next);
int q4_guide_delete(q4_guide* g);                       /* Q4_ERR_ARG while attached to a live model */
/* NULL: off. Q4_ERR_ARG: vocabulary != the model's, or a Transformer the library did not build. Sets the whole state ring to NONE. Graphs are captured
 * again only when the guide goes from off to on or back (another guide rewrites a small device block in stream order). */
int q4_set_guide(Transformer* t, const q4_guide* g);
const q4_guide* q4_get_guide(const Transformer* t);
int q4_get_guide_states(const Transformer* t, int first_pos, int n, int* out);   /* synchronises, like q4_get_logprobs; Q4_ERR_ARG without a guide */
/* Op-level form of the launch: logits [n] halves (16-byte aligned), n == the guide's vocabulary; state_ring, tokens and pPos (one int) device-visible;
 * a position outside [0, Q4_MAX_SEQ_LEN) does nothing. For one device and one stream: the op keeps one small parameter block for the life of the
 * process, on the device that was current at its first call, and (like q4_guide_delete) orders itself against the current q4 stream only. */
int q4_guide_mask(q4_half* logits, int n, const q4_guide* g, int* state_ring, const int* tokens, const int* pPos);
/* The row form (a verify pass with q4_set_pass_stages on): rows r < n_rows of logits, `ld` halves apart, at positions pos_rows_dev[r] = pos_rows_dev[0] + r,
 * tokens read from tokens_view_dev (device, tokens by absolute position). Block r walks the automaton from state_ring[pos_rows_dev[0] - 1] over the view's
 * tokens up to its own position, stores state_ring[pos_rows_dev[r]] and masks row r with it: rows and states are byte for byte what n_rows calls of
 * q4_guide_mask at consecutive positions leave. Halves between n and ld are neither read nor written. Also Q4_ERR_ARG: n_rows outside 1 .. 8, ld < n, ld
 * not a multiple of 8. */
int q4_guide_mask_rows(q4_half* logits, int n, const q4_guide* g, int* state_ring, int ld, int n_rows, const int* tokens_view_dev, const int* pos_rows_dev);
/* Host only: the forced tokens from `state` -- while the state has exactly one live token, that token, and on to the state behind it (a per-state array
 * built once by q4_guide_new). At most max_draft ids into draft_out; the run ends behind an EOS (token 2), at a state with two or more live tokens, and is
 * empty for Q4_GUIDE_NONE, Q4_GUIDE_OFFTRACK or a state outside the guide. Returns the number of ids written. */
int q4_guide_forced_run(const q4_guide* g, int state, int max_draft, int* draft_out);

/* ---- sequence snapshots and prompt-prefix reuse (q4_snapshot.hip, q4_kv_copy.hip; not in the reference) --------------------------
 * Everything a sequence keeps is indexed by position -- the K / V cache [layer][seq_len][kv_dim], the token ring, the coin ring, the guide's state ring,
 * the log-probability records, the penalty window -- and the device keeps its own position. These entry points start a sequence somewhere else than at
 * position 0, over K / V rows that are already in place, and keep a prefix's rows to put them back later or into another model of the same checkpoint.
 * All of it is opt-in: a caller who uses none of them gets the launches, the graphs and the tokens it got before. Nothing is added to the decode step. */
typedef struct q4_snapshot q4_snapshot;                 /* opaque, device-resident, immutable */
struct q4_snapshot_info {                               /* (the record shares its name with the function that fills it: write `struct q4_snapshot_info`) */
    int n_pos;                                          /* positions [0, n_pos) */
    int kv_format;                                      /* Q4_KV_FP16 / Q4_KV_FP8 */
    int n_layers, n_kv_heads, head_size;
    float rope_theta;
    unsigned long long fingerprint;                     /* of the checkpoint file: its header without seq_len, its size, its first and last 64 KiB; a model with
                                                           RoPE scaling: that, mixed with the fp32 bits of its frequencies (two settings that give the same frequencies interchange) */
    unsigned long long device_bytes;                    /* the packed rows */
    unsigned long long export_bytes;                    /* what q4_snapshot_export writes */
};
/* q4_reset_sequence that starts at start_pos: the same hand-off clearing, the same probation countdown, the guide ring to NONE; the device position and
 * SharedData::pos become start_pos, the ring receives tokens[0 .. num_tokens), and the K / V rows below start_pos stay as they are. The caller's contract:
 * those rows were computed from tokens[0 .. start_pos) -- by this model since its last q4_reset_sequence (start_pos below the current position is the
 * roll-back: regenerate an answer, edit the last turn), or put there by q4_snapshot_restore. Q4_ERR_ARG unless 0 <= start_pos <= num_tokens - 1 (the last
 * prompt token always runs: it produces the logits) and start_pos <= seq_len. start_pos = 0 is exactly q4_reset_sequence. Behind the resumed position a
 * guide starts at state 0, as behind any prompt; log-probability records below start_pos are left as they are. */
int q4_resume_sequence(RunState* s, const int* tokens, int num_tokens, int start_pos);
/* Synchronises the stream, then returns the largest start_pos that is safe for `tokens` as the model stands: the length of the common prefix of tokens
 * and the ring, capped by the positions the device has completed and by num_tokens - 1. 0 for a model whose rows are suspect: q4_handoff_status has
 * reported a time-out and no q4_reset_sequence has followed. A null pointer, num_tokens < 1 or a Transformer the library did not build: -Q4_ERR_ARG
 * (the one negative value it returns). */
int q4_common_prefix(const Transformer* t, const int* tokens, int num_tokens);
/* q4_generate_ids starting at start_pos (q4_generate_ids is the start_pos = 0 call of it). The loop draws one coin per step whether or not the step
 * samples, so start_pos coins are drawn from the sampler and discarded first: with the same seed a resumed sampled generation produces the full one's
 * tokens, and a reused Sampler stands at the same state after either. out_tokens holds the whole ring from index 0; timed_tokens is the reference's rule
 * over the steps this call ran (one less than their number). The retry after a hand-off time-out runs from position 0 with a full reset; so does a prompt
 * with an EOS token inside [1, start_pos), where the full loop would have stopped. A start_pos outside [0, num_prompt_tokens - 1] or above seq_len, or a
 * null pointer: -1.0 (like every failure of q4_generate_ids) with q4_last_error set, nothing touched. */
double q4_generate_ids_from(Transformer* t, Sampler* sampler, const int* prompt_tokens, int num_prompt_tokens, int steps, int start_pos,
                            int* out_tokens, int* timed_tokens, double* seconds);
/* Synchronises, then copies the K and V rows (an FP8 model's row exponents too) of positions [0, n_pos) of every layer into a packed device buffer:
 * [K|V][layer][n_pos][kv_dim] in the cache's own element type, then for an FP8 model [K|V][layer][n_kv_heads][n_pos] exponent bytes; keeps
 * tokens[0 .. n_pos) of the ring on the host. Q4_ERR_ARG unless 1 <= n_pos <= the positions the device has completed (SharedData::pos), and for a model
 * whose rows are suspect (q4_common_prefix). An FP8 model's fp16 staging rows are the current position's and are not part of a snapshot. */
int q4_snapshot_new(q4_snapshot** out, const Transformer* t, int n_pos);
/* Stream-ordered on the q4 stream: copies the rows back into positions [0, n_pos) of t, which may be another Transformer of the same checkpoint, also
 * one opened with another seq_len. Does not move the position or touch the ring: follow with q4_resume_sequence or q4_generate_ids_from at any
 * start_pos <= n_pos, with tokens that begin with the snapshot's. The restored prefix counts as a prompt: the guide ring is NONE there, so the automaton
 * starts at state 0 behind it, as behind any prompt; log-probability records below n_pos are left as they are. Q4_ERR_ARG, nothing copied: another
 * checkpoint or other RoPE frequencies (fingerprint), geometry (layers, kv heads, head size), rope_theta or K / V format, or n_pos above t's seq_len. */
int q4_snapshot_restore(Transformer* t, const q4_snapshot* s);
int q4_snapshot_delete(q4_snapshot* s);                 /* synchronises the q4 stream first: a restore may still be reading */
int q4_snapshot_info(const q4_snapshot* s, struct q4_snapshot_info* out);
int q4_snapshot_tokens(const q4_snapshot* s, int* out); /* out: n_pos ints */
/* The serialised form, little-endian: a 48-byte header {u32 magic "Q4SN", u32 version 1, i32 kv_format, i32 n_layers, i32 n_kv_heads, i32 head_size,
 * i32 n_pos, f32 rope_theta, u64 fingerprint, u64 payload_bytes}, n_pos i32 tokens, then the packed rows as above. q4_snapshot_export writes
 * export_bytes bytes (a smaller capacity: Q4_ERR_ARG); q4_snapshot_import checks with q4_snapshot_check first, then allocates and uploads.
 * q4_snapshot_check touches no GPU: the magic, the version, kv_format in {0, 1}, n_layers / n_kv_heads / head_size in [1, 65536], n_pos in
 * [1, Q4_MAX_SEQ_LEN], a finite rope_theta, and `bytes` exactly the size the header implies -- computed in 64 bits with overflow checks before anything
 * is allocated; a truncated, padded, negative-count or overflowing blob is Q4_ERR_ARG. out may be NULL. */
int q4_snapshot_export(const q4_snapshot* s, void* host, size_t capacity);
int q4_snapshot_import(q4_snapshot** out, const void* host, size_t bytes);
int q4_snapshot_check(const void* host, size_t bytes, struct q4_snapshot_info* out);
/* Op-level form of the copy launch (q4_kv_copy.hip): run r < outer moves run_bytes bytes from src + r * src_stride to dst + r * dst_stride on the q4
 * stream -- 16-byte accesses where source and destination share their offset from a 16-byte boundary, bytes elsewhere; any alignment, 64-bit offsets.
 * Q4_ERR_ARG without a launch: a null pointer, a negative argument, run_bytes above either stride when outer > 1, source and destination ranges (first
 * byte of the first run to last byte of the last) that overlap. */
int q4_copy_runs(void* dst, const void* src, long long outer, long long dst_stride, long long src_stride, long long run_bytes);

/* ---- batched decoding (q4_batch.hip; not in the reference) ------------------------------------------
 * A batch holds up to Q4_BATCH_MAX_SLOTS sequences ("slots") over ONE Transformer's weights; one pass advances every open slot by one position on one read
 * of the weights (the rows of a prompt pass, each row another sequence). A slot owns an fp16 K / V cache of the model's geometry, a token ring, a position,
 * a seed and a logits row. Everything a slot produces -- tokens, K / V rows, the logits of its last position -- is byte for byte what the same checkpoint
 * produces when it runs that sequence alone (q4_generate_ids with rng_seed = the slot's seed), whatever the other slots do. The model's own sequence (its
 * cache, ring, position, logits) is not touched. Passes run eagerly on the q4 stream; no captured graph contains one. There is no EOS rule: a host closes
 * a slot when it has seen enough. Delete a batch before its Transformer.
 * Admitted (q4_batch_covers; anything else: Q4_ERR_UNSUPPORTED_SIZE from q4_batch_new, nothing launched): dim 4096 in 128-wide heads -- Llama-2-7B's layer
 * shape, or the grouped-query one with four query heads per K / V head and a hidden size whose down projection runs the shared-half-slot form (Mistral-7B,
 * Llama-3-8B) --, a vocabulary that is a multiple of 8, the fp16 cache, no guide, no log-probability records. A step under a Sampler with a logit stage on
 * (sampling controls, bias, DRY, adaptive truncation), with a guide or records switched on since, at a fusion level below 3, or with a temperature the row
 * sampler does not take (q4_verify_sample_rows: vocabulary <= 32768, a finite temperature > 0) is refused the same way. A call that returns Q4_ERR_HIP
 * leaves the batch unusable: delete it. */
#define Q4_BATCH_MAX_SLOTS 8
typedef struct q4_batch q4_batch;                       /* opaque */
int q4_batch_covers(const Transformer* t);              /* 1 where q4_batch_new would build a batch, else 0 */
/* n_slots in 1 .. Q4_BATCH_MAX_SLOTS (else Q4_ERR_ARG); allocates n_slots caches of 2 x n_layers x seq_len x kv_dim halves and the pass's scratch, and
 * releases what it had allocated when an allocation fails (Q4_ERR_ALLOC). The caches start zeroed. */
int q4_batch_new(q4_batch** out, Transformer* t, int n_slots);
int q4_batch_delete(q4_batch* b);                       /* synchronises the q4 stream first */
/* Opens a closed slot at position 0 on prompt[0 .. n_prompt): while the slot is inside its prompt its row carries the next prompt token and the token
 * computed for that row is discarded, as a prompt step does; the pass at position n_prompt - 1 produces the first generated token. seed: the slot's coin
 * stream, one coin per position from 0 (q4_generate_ids' rule). Q4_ERR_ARG: a null pointer, a slot outside the batch or already open, n_prompt outside
 * 1 .. seq_len, a token outside the vocabulary. */
int q4_batch_open(q4_batch* b, int slot, const int* prompt, int n_prompt, unsigned long long seed);
/* Opens a closed slot behind a prefix someone already ingested: the snapshot's rows are copied into the slot's cache (q4_kv_copy.hip's launch, in stream
 * order) and the slot starts at position n_pos of the snapshot on prompt[0 .. n_prompt), whose first n_pos tokens must be the snapshot's and n_prompt > n_pos;
 * the coin stream stands where n_pos steps leave it. This is how a host uses prompt passes on the model's own sequence for long prompts. Q4_ERR_ARG:
 * q4_batch_open's, q4_snapshot_restore's (fingerprint, geometry, rope_theta, K / V format, n_pos above seq_len), or a prompt that does not begin with the
 * snapshot's tokens. */
int q4_batch_restore(q4_batch* b, int slot, const q4_snapshot* s, const int* prompt, int n_prompt, unsigned long long seed);
int q4_batch_close(q4_batch* b, int slot);              /* the slot's rows and logits stay readable until it is opened again; Q4_ERR_ARG: not open */
/* Several prompt positions of a slot per pass (chunked prefill), opt-in. max_rows_per_slot in 1 .. Q4_BATCH_MAX_SLOTS, else Q4_ERR_ARG and nothing
 * changes; the default 1 is one row per slot, launch for launch what a batch without this call runs. May be changed between passes. Above 1 the rows a pass
 * has spare -- Q4_BATCH_MAX_SLOTS minus the open slots -- go to slots inside their prompts (q4_batch_plan_rows); everything a slot produces stays byte
 * for byte the run alone's. q4_batch_get_prefill: the value in force (negative: -Q4_ERR_ARG). */
int q4_batch_set_prefill(q4_batch* b, int max_rows_per_slot);
int q4_batch_get_prefill(const q4_batch* b);
/* The schedule of one pass, a pure host function (no device call; q4_batch_step and q4_batch_generate plan every pass with it). open / pos / n_prompt
 * [n_slots]: per slot whether it is open, its position, its prompt length. rows_per_slot [n_slots] receives the rows each slot takes: 1 for every open
 * slot; then, in slot order, the spare rows to open slots with pos < n_prompt - 1, each up to min(max_rows_per_slot, n_prompt - pos) rows in all while
 * spare rows last. A slot's rows are the consecutive positions pos .. pos + rows - 1, adjacent and ascending in the pass, slots in slot order; the last may
 * be the generating row n_prompt - 1. Returns the pass's row count (0 .. Q4_BATCH_MAX_SLOTS), or -Q4_ERR_ARG: a null pointer, n_slots or
 * max_rows_per_slot outside 1 .. Q4_BATCH_MAX_SLOTS. */
int q4_batch_plan_rows(const int* open, const int* pos, const int* n_prompt, int n_slots, int max_rows_per_slot, int* rows_per_slot);
/* One pass over the weights: every open slot advances by one position -- a slot inside its prompt by up to q4_batch_set_prefill's rows, when the pass
 * has rows to spare. A slot produces at most one token per pass: only its last row can be a generating row. tokens_out [Q4_BATCH_MAX_SLOTS]: the slot's
 * generated token, or -1 for a closed slot, a slot outside the batch and a slot still inside its prompt. A row standing where the step's attention has no
 * row form (without graphs: positions 256 .. 510) refuses the whole pass with Q4_ERR_UNSUPPORTED_SIZE, nothing moved. sampler: temperature 0 greedy (the step's argmax and tie-breaking), else the
 * temperature / top-p sampler's row form with each slot's own coin; its rng_state is not used. Synchronises. Q4_ERR_ARG: a null pointer, or an open slot
 * that stands at seq_len (close it); nothing ran. No open slot: Q4_OK, nothing ran. */
int q4_batch_step(q4_batch* b, Sampler* sampler, int* tokens_out);
/* Up to `steps` passes queued back to back -- tokens stay on the device between passes -- and one synchronise at the end; stops early in front of a pass
 * in which an open slot would stand at seq_len. out [steps][Q4_BATCH_MAX_SLOTS]: row i is q4_batch_step's tokens_out of pass i (at most one token per
 * slot and pass, however many prompt positions the slot advanced by); *n_out: passes run. */
int q4_batch_generate(q4_batch* b, Sampler* sampler, int steps, int* out, int* n_out);
/* What the tests read; each synchronises. q4_batch_pos: the slot's position on the device (negative: -Q4_ERR_ARG) -- behind a pass it stands past every
 * row the slot took, one or several positions on; logits: the vocab halves of the slot's
 * last position (fp16 probabilities behind a sampled pass, as a sampled step leaves them); a K / V row of the slot's cache; the device addresses of the
 * slot's K and V caches, each [n_layers][seq_len][kv_dim] halves. */
int q4_batch_pos(const q4_batch* b, int slot);
int q4_batch_get_logits(const q4_batch* b, int slot, q4_half* host_out);
int q4_batch_get_kv_row(const q4_batch* b, int slot, int layer, int pos, q4_half* host_k, q4_half* host_v);
int q4_batch_cache(const q4_batch* b, int slot, q4_half** key_cache, q4_half** value_cache);

/* ---- context shift (q4_kv_shift.hip; not in the reference) ----------------------------------------
 * A sequence ends at seq_len: the K / V cache has that many rows. Context shift (the StreamingLLM / llama.cpp operation) keeps the first n_keep
 * positions, discards the n_discard = D positions behind them, slides everything above down by D and goes on at position n_pos - D: V rows move bit
 * for bit, K rows -- stored rotated -- are rotated by -D positions on the way, in ONE in-place launch off the per-token path; no weight is read.
 * The model then attends over rows that were computed WITH the discarded tokens in view: this is NOT what re-ingesting the surviving tokens gives.
 * What is guaranteed is the operation: deterministic, and specified exactly. With (c, s) = row D of the model's rotation table at pair index i,
 * a = float(k[i]), b = float(k[i + head_size/2]), every operation one IEEE fp32 operation:
 *   k'[i] = half_rne((a * c) + (b * s))      k'[i + head_size/2] = half_rne((b * c) - (a * s))
 * This holds for a model with RoPE scaling as well: row D of its table is the rotation of D positions for any per-pair frequency.
 * An FP8 K row is dequantised first (byte * 2^e, exactly fp16) and its rotated halves quantised again by the format's rule (new exponent, new
 * bytes); V bytes and exponents move as they are. Every shift therefore rounds the moved K rows once more (twice for FP8: to half and to e4m3), and
 * repeated shifts compound that. Opt-in: without these calls and without a setting, the launches, graphs, bits and return values are unchanged. */
/* Synchronises the q4 stream. With K0 = n_keep, D = n_discard, M = n_pos - K0 - D (M = 0: a pure truncation): K / V rows (FP8: and exponents) K0 + j <-
 * K0 + D + j, j < M, in every layer, K rotated as above; ring tokens[K0 + j] <- tokens[K0 + D + j], j < n_ring - K0 - D (n_ring covers the token the
 * last step chose and prompt tokens that still wait behind it); the device position and SharedData::pos become n_pos - D; with a guide attached the
 * state ring moves like the rows and entry n_pos - D - 1 receives the old entry n_pos - 1 (the automaton continues; nothing is cleared); with
 * log-probability records on they move like the rows (record p still describes the token at ring index p + 1); the hand-off counters and granules are
 * cleared as by q4_resume_sequence -- no probation countdown, no guide reset, rows_suspect stays. Untouched: rows and ring entries below K0, rows at
 * or above n_pos, the coin ring, the sampler, the logits, an FP8 model's staging rows, captured graphs. Rows [n_pos - D, n_pos) are unspecified
 * afterwards. Until the next q4_reset_sequence q4_common_prefix returns at most the smallest n_keep the sequence was shifted at: the rows above are no
 * longer "computed from tokens[0 .. start_pos)". q4_snapshot_new stays allowed: a snapshot of a shifted sequence restores that sequence's state, not
 * the state a fresh run over its tokens would reach.
 * Q4_ERR_ARG, nothing touched, no launch: a Transformer the library did not build or whose rows are suspect (q4_common_prefix); unless 0 <= n_keep,
 * 1 <= n_discard, n_keep + n_discard <= n_pos <= min(SharedData::pos, seq_len) and n_pos + 1 <= n_ring <= Q4_MAX_SEQ_LEN. (n_pos is explicit for the
 * reason q4_snapshot_new's is: after a stop at EOS up to Q4_MULTI_STEPS - 1 surplus steps may have run.) */
int q4_shift_context(Transformer* t, int n_pos, int n_keep, int n_discard, int n_ring);
/* The setting the library's own loops follow: n_discard = 0 is off (default). On: q4_generate_ids / q4_generate_ids_from / q4_generate accept steps
 * above seq_len, up to Q4_MAX_SEQ_LEN - 1; when the next step would run at position seq_len the loop waits for what is queued, calls
 * q4_shift_context(t, seq_len, n_keep, n_discard, seq_len + 1) and continues; out_tokens (steps + 1 ints) receives the whole history, evicted tokens
 * included; the prompt must fit as before; one coin is drawn per step; the shift's time is inside `seconds`; after a shift a hand-off time-out is not
 * retried (-1.0, q4_last_error set). q4_chat shifts before any step whose position would be seq_len and `steps` bounds the steps it runs.
 * Q4_ERR_ARG: a negative value, n_keep + n_discard > seq_len, a Transformer the library did not build. */
int q4_set_context_shift(Transformer* t, int n_keep, int n_discard);
int q4_get_context_shift(const Transformer* t, int* n_keep, int* n_discard);
/* "keep=4,discard=256": both keys optional in any order, keep defaults to 0. Q4_ERR_ARG and the outputs untouched: an unknown key, a malformed or
 * negative number, discard missing or 0. */
int q4_parse_context_shift(const char* text, int* n_keep, int* n_discard);
/* Synchronises; row `pos` of the model's own rotation table: head_size/2 (cos, sin) pairs of floats. Q4_ERR_ARG: pos outside [0, seq_len). */
int q4_get_rope_row(const Transformer* t, int pos, float* cos_sin);
/* Op-level form of the launch, on the q4 stream; device pointers. k, v: [n_layers][seq_len][n_kv_heads * head_size] halves (Q4_KV_FP16) or e4m3 bytes
 * (Q4_KV_FP8, then k_exp, v_exp: [n_layers][n_kv_heads][seq_len] exponent bytes); cos_sin: [head_size/2] (cos, sin) pairs, the rotation of n_discard
 * positions. Q4_ERR_ARG without a launch: a null k, v or cos_sin, null exponents or a base that is not 16-byte aligned with Q4_KV_FP8, a bad format,
 * a non-positive count (n_keep may be 0), an odd head size, an FP8 head size outside {64, 128, 256}, n_keep + n_discard > n_pos, n_pos > seq_len.
 * n_pos == n_keep + n_discard launches nothing. */
int q4_kv_shift(void* k, void* v, int8_t* k_exp, int8_t* v_exp, int kv_format, int n_layers, int seq_len, int n_kv_heads, int head_size,
                int n_pos, int n_keep, int n_discard, const float* cos_sin);

/* build_transformer(Transformer*, char* checkpoint_path, bool perplexity) llama2_q4.cu:408-426 (prints the
 * same "Model params" / "Loading Weights... done!" lines unless quiet), free_transformer :428-432 */
int q4_build_transformer(Transformer* t, const char* checkpoint_path, int perplexity);
void q4_free_transformer(Transformer* t);
void q4_set_quiet(int quiet);

/* opaque-handle convenience for FFI hosts that cannot lay out the structs (ctypes, cgo, JNI) */
Transformer* q4_transformer_new(const char* checkpoint_path, int perplexity, int* status);
void q4_transformer_delete(Transformer* t);
const Config* q4_transformer_config(const Transformer* t);
RunState* q4_transformer_state(Transformer* t);
TransformerWeights* q4_transformer_weights(Transformer* t);
Sampler* q4_sampler_new(int vocab_size, float temperature, float topp, unsigned long long rng_seed);
void q4_sampler_delete(Sampler* s);
/* generate()'s state reset, llama2_q4.cu:461-463: pos = 0, copy prompt tokens into the shared ring */
int q4_reset_sequence(RunState* s, const int* prompt_tokens, int num_prompt_tokens);
int q4_shared_pos(const RunState* s);
/* Fusion level 3 waits inside a launch with BOUNDED spins; one that ran out sets a device flag and the results from then on
 * are invalid. Synchronises the stream; Q4_OK, or -- once per incident -- Q4_ERR_HIP with q4_last_error() set, after which
 * the hand-off state is cleared and the library runs at fusion level 1 (no in-launch waits): redo the sequence
 * (q4_reset_sequence). q4_generate / q4_generate_ids / q4_perplexity_ids do that themselves, q4_chat reports and stops.
 * A loop built on q4_run_transformer should call it wherever it synchronises. q4_handoff_timeouts: incidents so far. */
int q4_handoff_status(const RunState* s);
int q4_handoff_timeouts(void);
/* Diagnostic: duration of the K / V stream per context position, in ticks of 10 ns, as q4_build_transformer measured it for this model on this device
 * (the split-context attention -> o-proj launch prices its held-back weight requests from it); 0: not measured (seq_len < 1024). */
double q4_kv_stream_price(const RunState* s);
int q4_shared_token(const RunState* s, int index);
/* parity dumps: synchronise, then copy fp16 logits / a KV row / the residual to the host */
int q4_get_logits(const Transformer* t, q4_half* host_out);
int q4_get_kv_row(const Transformer* t, int layer, int pos, q4_half* host_k, q4_half* host_v);   /* Q4_KV_FP8 models: the dequantised halves */
int q4_get_logits_array(const Transformer* t, int num_pos, float* host_out);

/* ---- host drivers (llama2_q4.cu:436-601, perplexity.h) ---------------------------------------- */
struct Tokenizer;
/* generate(Transformer*, Tokenizer*, Sampler*, char* prompt, int steps) llama2_q4.cu:436-492.
 * Returns the achieved tok/s it printed; timed_tokens/seconds optionally returned. */
double q4_generate(Transformer* t, struct Tokenizer* tokenizer, Sampler* sampler, const char* prompt, int steps,
                   int* timed_tokens, double* seconds);
/* token-id variant used by benches/tests when no tokenizer file is present: same loop, same timing rule,
 * no printing. out_tokens (steps+1 ints, may be NULL) receives the token ring. Returns tokens/s. */
double q4_generate_ids(Transformer* t, Sampler* sampler, const int* prompt_tokens, int num_prompt_tokens,
                       int steps, int* out_tokens, int* timed_tokens, double* seconds);
/* chat(...) llama2_q4.cu:507-601 */
void q4_chat(Transformer* t, struct Tokenizer* tokenizer, Sampler* sampler, const char* cli_user_prompt,
             const char* cli_system_prompt, int steps);
/* softmax / compute_perplexity perplexity.h:3-51 (host math) */
void q4_softmax_f32(float* x, int size);
float compute_perplexity(const int* tokens, float* logits, int num_tokens, int vocab_size);
/* get_dataset_perplexity perplexity.h:57-97, parseDataSetAndComputePreplexity :99-139 */
float q4_get_dataset_perplexity(char* dataset, struct Tokenizer* tokenizer, Transformer* t, Sampler* sampler);
double q4_parse_dataset_and_compute_perplexity(const char* textFileName, struct Tokenizer* tokenizer,
                                               Transformer* t, Sampler* sampler);
/* teacher-forced logits for given token ids (perplexity path without a tokenizer): runs num_tokens steps with
 * copyLogits, returns perplexity of targets[i] under step i's logits. Always per token: the fp32 logits_array path is the reference's (one copy per
 * step), and q4_set_pass_logprobs does not change it -- q4_score_ids below is the call that takes passes. */
float q4_perplexity_ids(Transformer* t, Sampler* sampler, const int* tokens_with_bos, int num_tokens);
/* Teacher-forced scoring without the (seq_len, vocab) fp32 array -- works on a model built with perplexity = 0: logprobs_out[i] is the log-probability of
 * tokens_with_bos[i + 1] under step i's logits, i < num_tokens <= seq_len - 1 (more: Q4_ERR_ARG). The steps are queued like generate()'s prompt steps
 * (q4_steps_that_fit / q4_run_transformer_steps), one synchronise at the end, one retry after a timed-out hand-off. Records are switched on with
 * top_k = 0 for the call if they were off, and the setting is put back -- the ring and the graphs with the record launch then live for one call (each
 * such call captures them again, q4_graph_captures counts it): a host that scores repeatedly calls q4_set_logprobs(t, 0) once beforehand.
 * With q4_set_pass_logprobs on, wherever a prompt pass is admitted (q4_set_prompt_ingest; every position of this call is prompt-only, so a pass may take
 * the last one too) up to 8 positions go out as one pass over the weights; a remainder of one position, positions at or above the bound of
 * q4_set_pass_context and models the passes do not cover keep their steps. logprobs_out, the records with K > 0, RunState::logits and the position
 * afterwards are the stepwise call's, byte for byte; q4_prompt_passes counts these passes too. */
int q4_score_ids(Transformer* t, Sampler* s, const int* tokens_with_bos, int num_tokens, float* logprobs_out);

/* ---- tokenizer.h:1-223 ------------------------------------------------------------------------ */
struct Tokenizer* q4_tokenizer_new(const char* tokenizer_path, int vocab_size);   /* build_tokenizer :35-59 */
void q4_tokenizer_delete(struct Tokenizer* t);                                     /* free_tokenizer :61-66 */
/* encode :102-223; tokens must hold strlen(text)+3 ints */
int q4_tokenizer_encode(struct Tokenizer* t, const char* text, int bos, int eos, int* tokens, int* n_tokens);
const char* q4_tokenizer_decode(struct Tokenizer* t, int prev_token, int token);   /* decode :68-79 */
int q4_tokenizer_max_token_length(const struct Tokenizer* t);
/* raw bytes of a vocabulary entry as the file holds them (may contain NUL; not terminated): what a guide compiler lifts a byte automaton over */
int q4_tokenizer_piece(const struct Tokenizer* t, int id, const char** bytes, int* len);

/* ---- CLI: main() llama2_q4.cu:622-720 behind a callable (the llama2_q4 executable calls this) --- */
int q4_main(int argc, char** argv);
/* the flag parser alone (llama2_q4.cu:624-690), for tests: fills the struct, returns 0, or 1 where the
 * reference would call error_usage() */
typedef struct {
    const char* checkpoint_path;
    const char* tokenizer_path;
    const char* dataset_path;
    int steps;
    const char* prompt;
    int perplexity;
    float temperature;
    float topp;
    unsigned long long rng_seed;
    const char* mode;
    const char* system_prompt;
    int seed_from_time;
} q4_cli_args;
int q4_parse_args(int argc, char** argv, q4_cli_args* out);

/* ---- measurement helpers (bench.py; not part of the reference surface) ------------------------ */
/* Launch `kernel_id` `iters` times over a ring of `ring` distinct weight sets (defeats the 256 MiB Infinity
 * Cache), each launch bracketed by dispatch timestamps (hipExtLaunchKernel start/stop events on the q4 stream);
 * returns the average pure kernel duration in microseconds, <0 on error. The ring is layers[i % ring] of `w`.
 *   0: fused rmsnorm + gate/up + SiLU (the decode path's dominant kernel)   1: plain int4 GEMV dim->hidden (gate)
 *   2: plain int4 GEMV hidden->dim (down, accum)   3: fused rmsnorm + qkv + rope   4: o-proj (accum)
 *   5: fp16 classifier (ring ignored)  */
double q4_bench_kernel(int kernel_id, const Config* p, RunState* s, const TransformerWeights* w, int iters,
                       double* min_us, double* max_us);
/* Steady-state cost of one launch of kernel_id INSIDE a hipGraph (kernel + boundary, what the decode loop pays):
 * `iters` launches over the ring of layers are captured into one graph and replayed `reps` times; wall-clock
 * microseconds per launch. ids as above, plus 6: attention, 7: rmsnorm, 8: argmax, 9: embedding copy. */
double q4_bench_kernel_graph(int kernel_id, const Config* p, RunState* s, const TransformerWeights* w, int iters,
                             int reps);
/* Average duration of one launch class INSIDE the eager decode network (inputs produced by the previous kernel,
 * caches as the token loop leaves them): runs `tokens` greedy decode steps from the current position with dispatch
 * timestamps on the launches in time_mask | report_mask, statistics over report_mask (1 qkv, 2 attention, 4 o-proj, 8 gate/up, 16 down,
 * 32 final norm + classifier, 64 embedding); microseconds, <0 on error. This is the duration bench.py's roofline
 * uses and the one `rocprofv3 --kernel-trace` reports for `bench.py --no-graphs`. */
double q4_bench_in_network(int time_mask, int report_mask, const Config* p, RunState* s, const TransformerWeights* w,
                           int tokens, double* min_us, double* max_us, int* launches);
int q4_device_info(char* name, int name_len, int* cu_count, size_t* hbm_bytes);

#ifdef __cplusplus
}
#endif
#endif /* LLAMA2_Q4_H */
