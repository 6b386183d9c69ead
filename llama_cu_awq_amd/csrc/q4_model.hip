// q4_model.hip -- the library's globals, stream and memory entry points, the per-model record, the loader, build and free.
// Mirrors llama2_q4.cu:38-202 (memory + loader), :408-432 (build_transformer, free_transformer).
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stdlib.h>
#include <string.h>
#include <math.h>
#include <chrono>
#include <type_traits>
#include <vector>
#include "q4_model.h"
#include "prompt_pass.h"
#include "spec_verify.h"
#include "option_text.h"

namespace q4 {

hipStream_t g_stream = nullptr;
int g_fusion = 5;
int g_kv_format = Q4_KV_FP16;
q4_rope_scaling g_rope_scaling = {};          // q4_set_rope_scaling; a CUSTOM setting's inv_freq points at g_rope_custom
static float g_rope_custom[Q4_ROPE_MAX_PAIRS];
int g_multi_steps = Q4_MULTI_STEPS;   // greedy steps per graph replay in the token loops (profiling build: q4_set_gemv_early(7, n))
int g_use_graphs = 1;
int g_quiet = 0;
char g_last_error[512] = "";
hipEvent_t g_ev_start = nullptr, g_ev_stop = nullptr;

int hip_fail(hipError_t e, const char* what, const char* file, int line) {
    snprintf(g_last_error, sizeof(g_last_error), "%s:%d: %s -> %s", file, line, what, hipGetErrorString(e));
    fprintf(stderr, "llama2_q4: HIP error %s\n", g_last_error);
    return Q4_ERR_HIP;
}

Models& models() { static Models m; return m; }

int lds_opt_in(const void* kernel, size_t bytes) {
    if (bytes <= 64 * 1024) return Q4_OK;
    static std::map<std::pair<const void*, int>, size_t> opted;
    int dev = 0;
    Q4_HIP(hipGetDevice(&dev));
    size_t& have = opted[{kernel, dev}];
    if (bytes > have) {
        Q4_HIP(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
        have = bytes;
    }
    return Q4_OK;
}

static size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

size_t qweight_bytes(int height, int width, size_t* wb, size_t* zb, size_t* sb) {
    // llama2_q4.cu:82-98
    size_t packed_wt_height = (size_t)divUp(height, 32) * 4;
    size_t scales_height = (size_t)divUp(height, Q4_GROUP_SIZE);
    size_t packed_zeros_height = (size_t)divUp((int)scales_height, 8);
    *wb = packed_wt_height * width * sizeof(uint32_t);
    *zb = packed_zeros_height * width * sizeof(uint32_t);
    *sb = scales_height * width * sizeof(q4_half);
    return *wb + *zb + *sb;
}

// ---------------------------------------------------------------------------------------------------
// build_transformer: llama2_q4.cu:408-426 = header fread + malloc_weights (:106-134) +
// checkpoint_init_weights (:172-202) + malloc_run_state (:38-67)
static int read_to_device(void* dst, FILE* fp, size_t bytes, void* scratch) {
    if (fread(scratch, 1, bytes, fp) != bytes) {                                   // readWeight :157-160
        printf("error reading weights");
        return Q4_ERR_IO;
    }
    Q4_HIP(hipMemcpy(dst, scratch, bytes, hipMemcpyHostToDevice));
    return Q4_OK;
}

struct SlabCursor {
    char* base;
    size_t off;
    void* take(size_t bytes) {
        void* p = base ? base + off : nullptr;
        off = align_up(off + bytes, 256);
        return p;
    }
};

// The tensor order of the file, written ONCE (checkpoint_init_weights :172-202): embedding, wcls, final norm; per layer q, k, v, o, up, gate, down
// and the two norm weights. visit(pointer, bytes) sees every read of the loader in file order -- a QWeight is three (uploadQWeight :162-170) -- and
// ends the walk by returning non-zero. The sizing pass, the pointer pass and the upload are visitors.
template <class Visit>
static int walk_tensors(TransformerWeights* w, const Config* p, Visit visit) {
    const int kv_dim = (p->dim * p->n_kv_heads) / p->n_heads;
    const size_t table = (size_t)p->vocab_size * p->dim * sizeof(q4_half), norm = (size_t)p->dim * sizeof(q4_half);
    Q4_TRY(visit(w->token_embedding_table, table));
    Q4_TRY(visit(w->wcls, table));
    Q4_TRY(visit(w->rms_final_weight, norm));
    for (int l = 0; l < p->n_layers; l++) {
        PerLayerWeight* L = &w->layers[l];
        const struct { QWeight* w; int height, width; } mats[] = {{&L->wq_q, p->dim, p->dim}, {&L->wq_k, p->dim, kv_dim}, {&L->wq_v, p->dim, kv_dim}, {&L->wq_o, p->dim, p->dim},
            {&L->wq_up, p->dim, p->hidden_dim}, {&L->wq_gate, p->dim, p->hidden_dim}, {&L->wq_down, p->hidden_dim, p->dim}};   // :191-192: up before gate
        for (const auto& mt : mats) {
            size_t wb, zb, sb;
            qweight_bytes(mt.height, mt.width, &wb, &zb, &sb);
            Q4_TRY(visit(mt.w->weight, wb)); Q4_TRY(visit(mt.w->zeros, zb)); Q4_TRY(visit(mt.w->scales, sb));
        }
        Q4_TRY(visit(L->rms_att_weight, norm));
        Q4_TRY(visit(L->rms_ffn_weight, norm));
    }
    return Q4_OK;
}
// hands every tensor its place in the slab (base null: sizes it only); `largest` = the largest single read
static void carve_weights(SlabCursor& c, TransformerWeights* w, const Config* p, size_t* largest) {
    (void)walk_tensors(w, p, [&](auto*& ptr, size_t bytes) {
        ptr = (std::remove_reference_t<decltype(ptr)>)c.take(bytes);
        if (bytes > *largest) *largest = bytes;
        return Q4_OK;
    });
}

// malloc_run_state :38-67. att holds n_heads*max(seq_len, dim) halves (the reference's n_heads*dim overflows
// for seq_len > dim); this build's attention does not use it at all.
static void carve_state(SlabCursor& c, RunState* s, const Config* p, Model& m) {
    const int kv_dim = (p->dim * p->n_kv_heads) / p->n_heads;
    s->x = (q4_half*)c.take((size_t)p->dim * sizeof(q4_half));
    s->xb = (q4_half*)c.take((size_t)p->dim * sizeof(q4_half));
    s->hb = (q4_half*)c.take((size_t)p->hidden_dim * sizeof(q4_half));
    s->q = (q4_half*)c.take((size_t)p->dim * sizeof(q4_half));
    s->att = (q4_half*)c.take(att_buffer_bytes(p));
    s->logits = (q4_half*)c.take((size_t)p->vocab_size * sizeof(q4_half));
    const size_t kv_elem = m.kv_format == Q4_KV_FP8 ? 1 : sizeof(q4_half);     // FP8: one byte per element, half the fp16 caches
    s->key_cache = (q4_half*)c.take(kv_elem * p->n_layers * p->seq_len * kv_dim);
    s->value_cache = (q4_half*)c.take(kv_elem * p->n_layers * p->seq_len * kv_dim);
    s->pos = (int*)c.take(sizeof(int));
    if (m.kv_format == Q4_KV_FP8) {
        m.k_exp = (int8_t*)c.take((size_t)p->n_layers * p->n_kv_heads * p->seq_len);
        m.v_exp = (int8_t*)c.take((size_t)p->n_layers * p->n_kv_heads * p->seq_len);
        m.k_row = (q4_half*)c.take((size_t)kv_dim * sizeof(q4_half));
        m.v_row = (q4_half*)c.take((size_t)kv_dim * sizeof(q4_half));
    }
}

// zeroed on the launch stream and waited for: a null-stream hipMemset returns before the device has finished, and nothing orders it
// before the first launches on a non-blocking g_stream -- a small model's first K / V rows could be zeroed AFTER they were written, and the
// hand-off words after the first launch of a caller who starts with q4_run_transformer instead of q4_reset_sequence
static void zero_on_stream(void* ptr, size_t bytes) {
    if (hipMemsetAsync(ptr, 0, bytes, g_stream) != hipSuccess || hipStreamSynchronize(g_stream) != hipSuccess) {
        (void)hipGetLastError();
        hipDeviceSynchronize();
        hipMemset(ptr, 0, bytes);
        hipDeviceSynchronize();
    }
}

// The split-context attention -> o-proj launch holds its o-proj role's weight requests back until the K / V stream of the context is about to end
// (layer_attn.h). What it needs is the stream's duration per context position ON THIS DEVICE, for THIS model's rows: measured here, once per model, with the
// product's own split-context attention launch at two context lengths (dispatch timestamps on the launch stream; the slope is the price, the fixed part of
// a launch drops out) -- instead of a constant measured on one box in round 5. A few hundred microseconds of build time; the run
// state is all zeros at this point and stays so (the launch writes xb and its scratch records only). Returns the price in 10 ns ticks, 0.0 without one.
static double measure_kv_price(const Config* p, RunState* s, unsigned* sync) {
    const int head_size = p->dim / p->n_heads;
    const int kv_dim = (p->dim * p->n_kv_heads) / p->n_heads;
    const int n2 = p->seq_len < 2048 ? p->seq_len : 2048, n1 = n2 / 2;
    if (n1 < 512 || p->n_heads > SYNC_MAX_HEADS || !(head_size == 64 || head_size == 128 || head_size == 256) || !s->att || g_stream == nullptr) return 0.0;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) { (void)hipGetLastError(); if (e0) hipEventDestroy(e0); return 0.0; }
    double t[2] = {0.0, 0.0};
    bool ok = true;
    for (int k = 0; k < 2 && ok; k++) {
        const int n = k ? n2 : n1;
        const int last = n - 1;
        ok = hipMemcpyAsync(s->pos, &last, sizeof(int), hipMemcpyHostToDevice, g_stream) == hipSuccess && hipStreamSynchronize(g_stream) == hipSuccess;
        double best = 1e30;
        for (int rep = 0; rep < 12 && ok; rep++) {       // the minimum of a dozen launches: the stream's own time, not a neighbour's
            // every launch on ANOTHER layer's rows (the token loop comes back to a layer after all the others: its rows come from HBM, while a
            // repeated read of one layer's 33 MB would come out of the 256 MB Infinity Cache at twice the rate)
            const size_t loff = (size_t)((rep * 7 + k * 3) % p->n_layers) * p->seq_len * kv_dim;
            g_ev_start = e0; g_ev_stop = e1;
            const int rc = launch_attention(s->xb, s->q, s->key_cache + loff, s->value_cache + loff, p->n_heads, head_size, p->n_heads / p->n_kv_heads, n, s->pos,
                                            (float*)s->att, att_buffer_bytes(p), p->n_heads <= SYNC_MAX_HEADS ? sync + SYNC_ARRIVE : nullptr);   // ONE launch: merged by each head's last block (the counters re-arm themselves)
            g_ev_start = g_ev_stop = nullptr;
            float ms = 0.f;
            ok = rc == Q4_OK && hipStreamSynchronize(g_stream) == hipSuccess && hipEventElapsedTime(&ms, e0, e1) == hipSuccess;
            if (ok && rep >= 2 && ms > 0.f && ms < best) best = ms;
        }
        t[k] = best;
    }
    const int zero = 0;
    (void)hipMemcpyAsync(s->pos, &zero, sizeof(int), hipMemcpyHostToDevice, g_stream);
    (void)hipMemsetAsync(s->xb, 0, (size_t)p->dim * sizeof(q4_half), g_stream);
    (void)hipStreamSynchronize(g_stream);
    hipEventDestroy(e0); hipEventDestroy(e1);
    if (!ok) { (void)hipGetLastError(); if (getenv("Q4_DEBUG_KV")) fprintf(stderr, "llama2_q4: kv price: measurement failed\n"); return 0.0; }
    const double ticks_per_pos = (t[1] - t[0]) * 1e-3 / (double)(n2 - n1) * 1e8;      // ms -> s -> 10 ns ticks
    // sanity: between a third of and three times the rows' bytes at 7.6 TB/s (what MI355X measures) -- outside that the measurement was disturbed and
    // the constant stands in
    const double nominal = (4.0 * kv_dim) / 7.6e12 * 1e8;
    if (getenv("Q4_DEBUG_KV")) fprintf(stderr, "llama2_q4: kv price: %d positions %.3f us, %d positions %.3f us -> %.4f ticks / position (nominal %.4f)\n", n1, t[0] * 1e3, n2, t[1] * 1e3, ticks_per_pos, nominal);
    return ticks_per_pos > nominal / 3.0 && ticks_per_pos < nominal * 3.0 ? ticks_per_pos : 0.0;
}

// What a snapshot of K / V rows is matched to its checkpoint by (q4_snapshot.hip): FNV-1a (64 bits) over the header with seq_len left out -- the rows of a
// position do not depend on it, and a snapshot may be restored into a model of the same file opened with another context length --, the file's size, and
// the file's first and last 64 KiB behind the header. Leaves the file positioned behind the header, where the loader expects it. 0 is never returned.
static unsigned long long checkpoint_fingerprint(FILE* file, const Config* p) {
    unsigned long long h = 0xcbf29ce484222325ull;
    auto mix = [&h](const void* data, size_t n) {
        const unsigned char* b = (const unsigned char*)data;
        for (size_t i = 0; i < n; i++) { h ^= b[i]; h *= 0x100000001b3ull; }
    };
    Config c = *p;
    c.seq_len = 0;
    mix(&c, sizeof(c));
    const long header = (long)sizeof(Config), window = 64 * 1024;
    long size = 0;
    if (fseek(file, 0, SEEK_END) == 0) size = ftell(file);
    if (size < header) size = header;
    const long long size64 = size;
    mix(&size64, sizeof(size64));
    std::vector<unsigned char> buf(window);
    const long first = size - header < window ? size - header : window;
    if (first > 0 && fseek(file, header, SEEK_SET) == 0) mix(buf.data(), fread(buf.data(), 1, (size_t)first, file));
    const long last_at = size - window > header ? size - window : header;
    if (size - last_at > 0 && fseek(file, last_at, SEEK_SET) == 0) mix(buf.data(), fread(buf.data(), 1, (size_t)(size - last_at), file));
    (void)fseek(file, header, SEEK_SET);
    return h ? h : 1;
}

// what q4_set_rope_scaling, q4_parse_rope_scaling and q4_rope_inv_freq accept (llama2_q4.h)
static bool rope_scaling_ok(const q4_rope_scaling* s) {
    if (!s || s->kind == Q4_ROPE_NONE) return true;
    const bool factor_ok = isfinite(s->factor) && s->factor >= 1.0f;
    switch (s->kind) {
        case Q4_ROPE_LINEAR: return factor_ok;
        case Q4_ROPE_LLAMA3:
            return factor_ok && isfinite(s->low_freq_factor) && isfinite(s->high_freq_factor) && s->low_freq_factor > 0.0f &&
                   s->low_freq_factor < s->high_freq_factor && s->original_max_position >= 1;
        case Q4_ROPE_CUSTOM:
            if (s->n_freqs < 1 || s->n_freqs > Q4_ROPE_MAX_PAIRS || !s->inv_freq) return false;
            for (int i = 0; i < s->n_freqs; i++)
                if (!isfinite(s->inv_freq[i]) || s->inv_freq[i] < 0.0f) return false;
            return true;
    }
    return false;
}

// the text form q4_parse_rope_scaling reads ("Model params" prints it); CUSTOM has none
static void rope_scaling_text(const q4_rope_scaling& r, char* out, size_t n) {
    switch (r.kind) {
        case Q4_ROPE_LINEAR: snprintf(out, n, "linear,factor=%g", r.factor); break;
        case Q4_ROPE_LLAMA3:
            snprintf(out, n, "llama3,factor=%g,low=%g,high=%g,orig=%d", r.factor, r.low_freq_factor, r.high_freq_factor, r.original_max_position);
            break;
        case Q4_ROPE_CUSTOM: snprintf(out, n, "custom,n_freqs=%d", r.n_freqs); break;
        default: snprintf(out, n, "none");
    }
}

// The scaled model's frequencies, their device copy, its (mandatory) table, and its fingerprint: the checkpoint's mixed with the frequencies' fp32 bits
static int build_scaled_rope(Model& m, const Config* p) {
    const int head_size = p->dim / p->n_heads, hp = head_size / 2;
    if (head_size < 2 || (head_size & 1)) {
        snprintf(g_last_error, sizeof(g_last_error), "rope scaling: head size %d is not even", head_size);
        return Q4_ERR_ARG;
    }
    if (m.rope.kind == Q4_ROPE_CUSTOM && m.rope.n_freqs != hp) {
        snprintf(g_last_error, sizeof(g_last_error), "rope scaling: %d custom frequencies for a head size of %d (needs %d)", m.rope.n_freqs, head_size, hp);
        return Q4_ERR_ARG;
    }
    m.inv_freq.resize(hp);
    if (q4_rope_inv_freq(&m.rope, head_size, p->rope_theta, m.inv_freq.data())) {
        snprintf(g_last_error, sizeof(g_last_error), "rope scaling: no frequencies for head size %d and rope_theta %g", head_size, p->rope_theta);
        return Q4_ERR_ARG;
    }
    m.rope.inv_freq = nullptr;     // (pointed at g_rope_custom, which the next q4_set_rope_scaling rewrites)
    if (hipMalloc((void**)&m.inv_freq_dev, hp * sizeof(float)) != hipSuccess) {
        (void)hipGetLastError();
        m.inv_freq_dev = nullptr;
        snprintf(g_last_error, sizeof(g_last_error), "rope scaling: no device memory for %d frequencies", hp);
        return Q4_ERR_ALLOC;
    }
    Q4_HIP(hipMemcpy(m.inv_freq_dev, m.inv_freq.data(), hp * sizeof(float), hipMemcpyHostToDevice));
    Q4_TRY(rope_table_build_freqs(&m.rope_table, p->seq_len, head_size, m.inv_freq_dev));
    unsigned long long h = 0xcbf29ce484222325ull;
    auto mix = [&h](const void* data, size_t n) {
        const unsigned char* b = (const unsigned char*)data;
        for (size_t i = 0; i < n; i++) { h ^= b[i]; h *= 0x100000001b3ull; }
    };
    mix(&m.fingerprint, sizeof(m.fingerprint));
    mix(m.inv_freq.data(), hp * sizeof(float));
    m.fingerprint = h ? h : 1;
    return Q4_OK;
}

// everything behind the header and the record's registration; the caller closes the file and, on failure, leaves through q4_free_transformer
static int load_model(Transformer* t, Model& m, FILE* file, int perplexity) {
    const Config* p = &t->config;
    TransformerWeights* w = &t->weights;
    // pass 1 sizes the weight slab, pass 2 hands out pointers; staging buffer = the largest single read (the reference sizes it
    // max(vocab, hidden) * dim halves, :176, which a q/o matrix outgrows when dim > 4 * max(vocab, hidden))
    size_t scratch_size = 0;
    SlabCursor dry = {nullptr, 0};
    carve_weights(dry, w, p, &scratch_size);
    if (hipMalloc(&m.weights, dry.off) != hipSuccess) { printf("malloc failed!\n"); return Q4_ERR_ALLOC; }
    SlabCursor cur = {(char*)m.weights, 0};
    carve_weights(cur, w, p, &scratch_size);

    void* scratch = nullptr;
    if (hipHostMalloc(&scratch, scratch_size, hipHostMallocDefault) != hipSuccess) scratch = nullptr;
    const bool scratch_pinned = scratch != nullptr;
    if (!scratch) scratch = malloc(scratch_size);
    if (!g_quiet) printf("\nLoading Weights... ");
    int rc = walk_tensors(w, p, [&](auto*& ptr, size_t bytes) { return read_to_device(ptr, file, bytes, scratch); });
    if (scratch_pinned) hipHostFree(scratch); else free(scratch);
    if (rc) return rc;
    if (!g_quiet) printf("done!\n");
    if ((rc = down_strip_prepare()) || (rc = cls_strip_prepare()) || (rc = ffn_pair_prepare())) return rc;   // (an attribute call: before any graph capture)

    RunState* s = &t->state;
    SlabCursor sd = {nullptr, 0};
    carve_state(sd, s, p, m);
    if (hipMalloc(&m.state, sd.off) != hipSuccess) { printf("malloc failed for allocaing run state!\n"); return Q4_ERR_ALLOC; }
    zero_on_stream(m.state, sd.off);
    cur = {(char*)m.state, 0};
    carve_state(cur, s, p, m);
    m.att_bytes = att_buffer_bytes(p);
    if (hipHostMalloc(&m.shared, sizeof(SharedData), hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess) {   // cudaMallocHost :50
        printf("malloc failed for allocaing run state!\n");
        return Q4_ERR_ALLOC;
    }
    s->shared_data = (SharedData*)m.shared;
    s->shared_data->pos = 0;
    memset((void*)s->shared_data->tokens, 0, sizeof(int) * 16);
    if (perplexity) {                                                              // :60-66
        if (hipMalloc(&m.logits_array, sizeof(float) * p->seq_len * p->vocab_size) != hipSuccess) {
            printf("malloc failed for allocaing logits_array!\n");
            return Q4_ERR_ALLOC;
        }
        s->logits_array = (float*)m.logits_array;
    }
    // fused QKV + RoPE epilogue (multi-head and grouped-query models alike): table of this model's own seq_len
    const auto rope_t0 = std::chrono::steady_clock::now();
    if (m.rope.kind != Q4_ROPE_NONE) Q4_TRY(build_scaled_rope(m, p));
    else Q4_TRY(rope_table_build(&m.rope_table, p->seq_len, p->dim / p->n_heads, p->rope_theta));
    if (getenv("Q4_DEBUG_ROPE"))     // (tools/bench_rope_scaling.py reads it: frequencies, allocation, the table launch and its synchronise)
        fprintf(stderr, "llama2_q4: rope table: %zu entries, scaling kind %d, built in %.3f ms\n", (size_t)p->seq_len * (p->dim / p->n_heads / 2), m.rope.kind,
                std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - rope_t0).count());
    const size_t sync_words = ffn_pair_sync_offset(p->dim) + ffn_pair_sync_words(p->dim, p->hidden_dim);
    if (hipMalloc((void**)&m.sync, sync_words * sizeof(unsigned)) == hipSuccess) {
        zero_on_stream(m.sync, sync_words * sizeof(unsigned));
        m.sync_words = sync_words;
        if (m.kv_format == Q4_KV_FP16) m.kv_price = measure_kv_price(p, s, m.sync);   // (prices the fp16 split-context attention -> o-proj launch, which an FP8 model never runs)
    } else {
        (void)hipGetLastError();    // no hand-off words: the network runs its five-launch sequence
        m.sync = nullptr;
    }
    // the greedy steps' screening copy of wcls, where the classifier runs as strips; without it (another shape, no memory left) the model decodes as before
    if (cls_screen_shape(p->dim, p->vocab_size) && cls_screen_build(&m.screen, w->wcls, p->dim, p->vocab_size) != Q4_OK) m.screen = ClsScreen{};
    return Q4_OK;
}

}  // namespace q4

using namespace q4;

extern "C" {

const char* q4_status_string(int status) {
    switch (status) {
        case Q4_OK: return "ok";
        case Q4_ERR_UNSUPPORTED_SIZE: return "Unsupported matmul size. Exiting";   // llama2_q4.cu:215
        case Q4_ERR_ALLOC: return "malloc failed!";                                // :131
        case Q4_ERR_IO: return "error reading weights";                            // :158
        case Q4_ERR_HIP: return "HIP runtime error";
        case Q4_ERR_ARG: return "invalid argument";
        case Q4_NOT_ADMITTED: return "not admitted";
    }
    return "unknown";
}
const char* q4_last_error(void) { return g_last_error; }

int q4_set_device(int device) {
    Q4_HIP(hipSetDevice(device));
    // LDS opt-ins of kernels the public matmuls may launch: attribute calls, made before any stream capture can begin
    int rc = down_strip_prepare();
    if (!rc) rc = cls_strip_prepare();
    return rc ? rc : cls_screen_prepare();
}
int q4_stream_create(q4_stream_t* out) {
    hipStream_t s;
    Q4_HIP(hipStreamCreate(&s));
    *out = (q4_stream_t)s;
    return Q4_OK;
}
// A stream restricted to the first `n_cus` compute units (hipExtStreamCreateWithCUMask): lets a host run replicas side by
// side on one GPU, and lets the tests run the in-launch hand-offs with fewer resident blocks than a whole device offers.
int q4_stream_create_masked(q4_stream_t* out, int n_cus) {
    int dev = 0, total = 0;
    Q4_HIP(hipGetDevice(&dev));
    Q4_HIP(hipDeviceGetAttribute(&total, hipDeviceAttributeMultiprocessorCount, dev));
    if (n_cus < 1 || n_cus > total) return Q4_ERR_ARG;
    uint32_t mask[16] = {};
    const int words = (total + 31) / 32;
    if (words > 16) return Q4_ERR_ARG;
    // CU bits are interleaved over the XCDs in the mask (bit i = CU i / 8 of XCD i % 8 on gfx950): taking the first n bits
    // spreads the stream over all XCDs
    for (int i = 0; i < n_cus; i++) mask[i >> 5] |= 1u << (i & 31);
    hipStream_t s;
    Q4_HIP(hipExtStreamCreateWithCUMask(&s, (uint32_t)words, mask));
    *out = (q4_stream_t)s;
    return Q4_OK;
}
int q4_stream_destroy(q4_stream_t s) {
    if ((hipStream_t)s == g_stream) g_stream = nullptr;
    attention_oproj_forget_stream((hipStream_t)s);
    Q4_HIP(hipStreamDestroy((hipStream_t)s));
    return Q4_OK;
}
void q4_set_stream(q4_stream_t s) { g_stream = (hipStream_t)s; }
q4_stream_t q4_get_stream(void) { return (q4_stream_t)g_stream; }
int q4_stream_synchronize(void) { Q4_HIP(hipStreamSynchronize(g_stream)); return Q4_OK; }
int q4_device_synchronize(void) { Q4_HIP(hipDeviceSynchronize()); return Q4_OK; }

int q4_malloc(void** dptr, size_t bytes) { Q4_HIP(hipMalloc(dptr, bytes)); return Q4_OK; }
int q4_free(void* dptr) { Q4_HIP(hipFree(dptr)); return Q4_OK; }
int q4_memcpy_h2d(void* dst, const void* src, size_t bytes) {
    Q4_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, g_stream));
    Q4_HIP(hipStreamSynchronize(g_stream));
    return Q4_OK;
}
int q4_memcpy_d2h(void* dst, const void* src, size_t bytes) {
    Q4_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, g_stream));
    Q4_HIP(hipStreamSynchronize(g_stream));
    return Q4_OK;
}
int q4_memset(void* dst, int value, size_t bytes) {
    Q4_HIP(hipMemsetAsync(dst, value, bytes, g_stream));
    return Q4_OK;
}

int q4_ffn_pair_covers(int dim, int hidden_dim) { return ffn_pair_covers(dim, hidden_dim) ? 1 : 0; }
// 1: captured graphs (USE_CUDA_GRAPHS, llama2_q4.cu:33); 0: eager launches with the exact context length (the reference's other path, :374);
// 2: eager launches with the graph path's sequence-length BIN -- what the graphs run, one launch at a time: the mode to profile in
// (rocprofv3 cannot trace inside a graph capture; with 0 the attention launch picks its form from the context length, not from the bin)
void q4_set_use_graphs(int enable) { g_use_graphs = enable == 2 ? 2 : enable ? 1 : 0; }
void q4_set_quiet(int quiet) { g_quiet = quiet; }

int q4_device_info(char* name, int name_len, int* cu_count, size_t* hbm_bytes) {
    int dev = 0;
    Q4_HIP(hipGetDevice(&dev));
    hipDeviceProp_t prop;
    Q4_HIP(hipGetDeviceProperties(&prop, dev));
    if (name && name_len > 0) snprintf(name, name_len, "%s (%s)", prop.name, prop.gcnArchName);
    if (cu_count) *cu_count = prop.multiProcessorCount;
    if (hbm_bytes) *hbm_bytes = prop.totalGlobalMem;
    return Q4_OK;
}

int q4_build_transformer(Transformer* t, const char* checkpoint_path, int perplexity) {
    memset(t, 0, sizeof(*t));
    FILE* file = fopen(checkpoint_path, "rb");
    if (!file) { printf("Couldn't open file %s\n", checkpoint_path); return Q4_ERR_IO; }   // :412
    if (fread(&t->config, sizeof(Config), 1, file) != 1) { printf("Invalid header size\n"); fclose(file); return Q4_ERR_IO; }
    Config* p = &t->config;
    if (!g_quiet)
        printf("\nModel params:- \ndim: %d \nhidden_dim: %d\nn_heads: %d\nn_kv_heads: %d\nn_layers: %d\nseq_len: %d\nvocab_size: %d\nrope_theta: %g\n",
               p->dim, p->hidden_dim, p->n_heads, p->n_kv_heads, p->n_layers, p->seq_len, p->vocab_size, p->rope_theta);   // :416-417
    if (!g_quiet && g_rope_scaling.kind != Q4_ROPE_NONE) {      // one more line, for a scaled model only
        char text[128];
        rope_scaling_text(g_rope_scaling, text, sizeof(text));
        printf("rope_scaling: %s\n", text);
    }
    if (p->dim <= 0 || p->n_heads <= 0 || p->n_kv_heads <= 0 || p->n_layers <= 0 || p->vocab_size <= 0 || p->seq_len <= 0 ||
        p->dim % p->n_heads || p->n_heads % p->n_kv_heads || (p->dim & 31) || (p->hidden_dim & 31) ||
        p->seq_len > Q4_MAX_SEQ_LEN) {
        printf("Unsupported model geometry\n");
        fclose(file);
        return Q4_ERR_UNSUPPORTED_SIZE;
    }
    t->weights.layers = (PerLayerWeight*)calloc(p->n_layers, sizeof(PerLayerWeight));   // malloc_weights :109
    t->weights.num_layers = p->n_layers;
    if (!t->weights.layers) { printf("malloc failed!\n"); fclose(file); return Q4_ERR_ALLOC; }
    // the first allocation exists: the record is registered, and from here every failure leaves through q4_free_transformer
    Model& m = models()[&t->state] = Model{};
    m.kv_format = g_kv_format;
    m.rope = g_rope_scaling;
    m.fingerprint = checkpoint_fingerprint(file, p);
    if (m.kv_format == Q4_KV_FP8 && !kv8_head_size_ok(p->dim / p->n_heads)) {
        snprintf(g_last_error, sizeof(g_last_error), "FP8 KV cache: head size %d is not supported (64, 128 or 256)", p->dim / p->n_heads);
        printf("%s\n", g_last_error);
        fclose(file);
        q4_free_transformer(t);
        return Q4_ERR_UNSUPPORTED_SIZE;
    }
    const int rc = load_model(t, m, file, perplexity);
    fclose(file);
    if (rc) q4_free_transformer(t);
    return rc;
}

void q4_free_transformer(Transformer* t) {                                        // :428-432
    if (!t) return;
    drop_graphs_of(&t->state);
    auto it = models().find(&t->state);
    if (it != models().end()) {
        Model& m = it->second;
        hipDeviceSynchronize();
        guide_release(&m);
        adaptive_release(&m);
        pass_release(&m);
        for (void* d : {m.weights, m.state, m.logits_array, (void*)m.rope_table, (void*)m.inv_freq_dev, (void*)m.sync, m.lp_ring, m.screen.base})
            if (d) hipFree(d);
        if (m.shared) hipHostFree(m.shared);
        models().erase(it);
    }
    free(t->weights.layers);
    memset(t, 0, sizeof(*t));
}

int q4_set_kv_format(int format) {
    if (format != Q4_KV_FP16 && format != Q4_KV_FP8) return Q4_ERR_ARG;
    g_kv_format = format;
    return Q4_OK;
}
int q4_get_kv_format(void) { return g_kv_format; }
int q4_kv_format_of(const RunState* s) { const Model* m = model_of(s); return m ? m->kv_format : Q4_KV_FP16; }

int q4_set_rope_scaling(const q4_rope_scaling* s) {
    if (!rope_scaling_ok(s) || (s && (s->kind < Q4_ROPE_NONE || s->kind > Q4_ROPE_CUSTOM))) return Q4_ERR_ARG;
    q4_rope_scaling r = {};
    if (s && s->kind != Q4_ROPE_NONE) {
        r.kind = s->kind;
        if (s->kind != Q4_ROPE_CUSTOM) r.factor = s->factor;
        if (s->kind == Q4_ROPE_LLAMA3) {
            r.low_freq_factor = s->low_freq_factor; r.high_freq_factor = s->high_freq_factor; r.original_max_position = s->original_max_position;
        }
        if (s->kind == Q4_ROPE_CUSTOM) {
            r.n_freqs = s->n_freqs;
            memmove(g_rope_custom, s->inv_freq, (size_t)s->n_freqs * sizeof(float));     // (the caller may hand back q4_get_rope_scaling's own pointer)
            r.inv_freq = g_rope_custom;
        }
    }
    g_rope_scaling = r;
    return Q4_OK;
}
int q4_get_rope_scaling(q4_rope_scaling* out) {
    if (!out) return Q4_ERR_ARG;
    *out = g_rope_scaling;
    return Q4_OK;
}
int q4_rope_scaling_of(const Transformer* t, q4_rope_scaling* out) {
    const Model* m = t ? model_of(&t->state) : nullptr;
    if (!m || !out) return Q4_ERR_ARG;
    *out = m->rope;
    out->inv_freq = m->inv_freq.empty() ? nullptr : m->inv_freq.data();
    return Q4_OK;
}
int q4_get_rope_inv_freq(const Transformer* t, float* out) {
    const Model* m = t ? model_of(&t->state) : nullptr;
    if (!m || !out || m->inv_freq.empty()) return Q4_ERR_ARG;
    memcpy(out, m->inv_freq.data(), m->inv_freq.size() * sizeof(float));
    return Q4_OK;
}
int q4_rope_inv_freq(const q4_rope_scaling* s, int head_size, float rope_theta, float* out) {
    if (!out || head_size < 2 || (head_size & 1) || !isfinite(rope_theta) || !(rope_theta > 0.0f) || !rope_scaling_ok(s)) return Q4_ERR_ARG;
    const int hp = head_size / 2, kind = s ? s->kind : Q4_ROPE_NONE;
    if (kind < Q4_ROPE_NONE || kind > Q4_ROPE_CUSTOM) return Q4_ERR_ARG;
    if (kind == Q4_ROPE_CUSTOM) {
        if (s->n_freqs != hp) return Q4_ERR_ARG;
        memmove(out, s->inv_freq, (size_t)hp * sizeof(float));
        return Q4_OK;
    }
    for (int i = 0; i < hp; i++) {
        const double f = pow((double)rope_theta, -(2.0 * i) / head_size);
        double r = f;
        if (kind == Q4_ROPE_LINEAR) {
            r = f / (double)s->factor;
        } else if (kind == Q4_ROPE_LLAMA3) {           // Hugging Face _compute_llama3_parameters
            const double factor = s->factor, low = s->low_freq_factor, high = s->high_freq_factor, orig = s->original_max_position;
            const double wl = 2.0 * M_PI / f;
            if (wl < orig / high) r = f;
            else if (wl > orig / low) r = f / factor;
            else {
                const double sm = (orig / wl - low) / (high - low);
                r = (1.0 - sm) * f / factor + sm * f;
            }
        }
        out[i] = (float)r;
    }
    return Q4_OK;
}
// "none" | "linear,factor=4" | "llama3,factor=8,low=1,high=4,orig=8192"
int q4_parse_rope_scaling(const char* text, q4_rope_scaling* out) {
    if (!text || !out) return Q4_ERR_ARG;
    const char* end = strchr(text, ',');
    if (!end) end = text + strlen(text);
    const size_t kl = (size_t)(end - text);
    q4_rope_scaling r = {};
    if (kl == 4 && !strncmp(text, "none", 4)) r.kind = Q4_ROPE_NONE;
    else if (kl == 6 && !strncmp(text, "linear", 6)) r.kind = Q4_ROPE_LINEAR;
    else if (kl == 6 && !strncmp(text, "llama3", 6)) r.kind = Q4_ROPE_LLAMA3;
    else return Q4_ERR_ARG;
    const char* const keys[] = {"factor", "low", "high", "orig"};
    const int n_keys = r.kind == Q4_ROPE_LINEAR ? 1 : r.kind == Q4_ROPE_LLAMA3 ? 4 : 0;
    int seen = 0;
    const char* p = *end ? end + 1 : end;
    if (*end && !*p) return Q4_ERR_ARG;                        // a trailing comma
    while (*p) {
        char key[OPTION_KEY_CAP], val[48];
        if (!next_option(&p, key, val, sizeof(val))) return Q4_ERR_ARG;
        int k = 0;
        while (k < n_keys && strcmp(key, keys[k])) k++;
        if (k == n_keys || (seen & (1 << k))) return Q4_ERR_ARG;
        seen |= 1 << k;
        if (!((val[0] >= '0' && val[0] <= '9') || val[0] == '.')) return Q4_ERR_ARG;     // (no sign, no leading blank, no "inf" / "nan")
        char* rest = nullptr;
        if (k == 3) {
            const long v = strtol(val, &rest, 10);
            if (*rest || v < 1 || v > 0x7fffffffL) return Q4_ERR_ARG;
            r.original_max_position = (int)v;
        } else {
            const float v = strtof(val, &rest);
            if (*rest || !isfinite(v)) return Q4_ERR_ARG;
            (k == 0 ? r.factor : k == 1 ? r.low_freq_factor : r.high_freq_factor) = v;
        }
    }
    if (seen != (1 << n_keys) - 1 || !rope_scaling_ok(&r)) return Q4_ERR_ARG;
    *out = r;
    return Q4_OK;
}

double q4_kv_stream_price(const RunState* s) { const Model* m = model_of(s); return m ? m->kv_price : 0.0; }

Transformer* q4_transformer_new(const char* checkpoint_path, int perplexity, int* status) {
    Transformer* t = (Transformer*)calloc(1, sizeof(Transformer));
    int rc = q4_build_transformer(t, checkpoint_path, perplexity);
    if (status) *status = rc;
    if (rc) { free(t); return nullptr; }
    return t;
}
void q4_transformer_delete(Transformer* t) {
    if (!t) return;
    q4_free_transformer(t);
    free(t);
}
const Config* q4_transformer_config(const Transformer* t) { return &t->config; }
RunState* q4_transformer_state(Transformer* t) { return &t->state; }
TransformerWeights* q4_transformer_weights(Transformer* t) { return &t->weights; }

int q4_get_logits(const Transformer* t, q4_half* host_out) {
    Q4_HIP(hipStreamSynchronize(g_stream));
    Q4_HIP(hipMemcpy(host_out, t->state.logits, (size_t)t->config.vocab_size * sizeof(q4_half), hipMemcpyDeviceToHost));
    return Q4_OK;
}
int q4_get_kv_row(const Transformer* t, int layer, int pos, q4_half* host_k, q4_half* host_v) {
    const Config* p = &t->config;
    const int kv_dim = (p->dim * p->n_kv_heads) / p->n_heads;
    const size_t off = (size_t)layer * p->seq_len * kv_dim + (size_t)pos * kv_dim;
    Q4_HIP(hipStreamSynchronize(g_stream));
    const Model* m = model_of(&t->state);
    if (m && m->kv_format == Q4_KV_FP8) {      // bytes * 2^e, exactly an fp16 number each
        const int head_size = p->dim / p->n_heads;
        std::vector<uint8_t> b(kv_dim);
        std::vector<int8_t> e(p->n_kv_heads);
        for (int which = 0; which < 2; which++) {
            const uint8_t* bytes = (const uint8_t*)(which ? t->state.value_cache : t->state.key_cache) + off;
            const int8_t* exps = (which ? m->v_exp : m->k_exp) + (size_t)layer * p->n_kv_heads * p->seq_len + pos;
            Q4_HIP(hipMemcpy(b.data(), bytes, (size_t)kv_dim, hipMemcpyDeviceToHost));
            Q4_HIP(hipMemcpy2D(e.data(), 1, exps, (size_t)p->seq_len, 1, (size_t)p->n_kv_heads, hipMemcpyDeviceToHost));
            q4_half* out = which ? host_v : host_k;
            for (int i = 0; i < kv_dim; i++) {
                const int E = (b[i] >> 3) & 15, M = b[i] & 7;
                const float mag = E ? ldexpf(1.0f + M / 8.0f, E - 7) : ldexpf(M / 8.0f, -6);      // OCP e4m3fn (the quantiser never writes a NaN byte)
                const _Float16 v = (_Float16)ldexpf((b[i] & 0x80) ? -mag : mag, e[i / head_size]);
                memcpy(&out[i], &v, sizeof(v));
            }
        }
        return Q4_OK;
    }
    Q4_HIP(hipMemcpy(host_k, t->state.key_cache + off, (size_t)kv_dim * sizeof(q4_half), hipMemcpyDeviceToHost));
    Q4_HIP(hipMemcpy(host_v, t->state.value_cache + off, (size_t)kv_dim * sizeof(q4_half), hipMemcpyDeviceToHost));
    return Q4_OK;
}
int q4_get_logits_array(const Transformer* t, int num_pos, float* host_out) {
    if (!t->state.logits_array) return Q4_ERR_ARG;
    Q4_HIP(hipStreamSynchronize(g_stream));
    Q4_HIP(hipMemcpy(host_out, t->state.logits_array, (size_t)num_pos * t->config.vocab_size * sizeof(float), hipMemcpyDeviceToHost));
    return Q4_OK;
}

}  // extern "C"
