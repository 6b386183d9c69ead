// q4_network.hip -- the per-token network: which launches a token's layers are (NetForms), run_network, and the measurement hooks on it.
// Mirrors llama2_q4.cu:286-340 (run_llama_network).
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <vector>
#include "q4_model.h"

using namespace q4;

// measurement knob (tools/lab/breakdown.py): leave out a class of launches to read its marginal cost inside the token
// graph. Results are garbage with any bit set; never set by the product path.
#ifdef Q4_PROFILING
static int g_skip = 0;
extern "C" void q4_set_skip_mask(int mask) { g_skip = mask; q4_reset_graphs(); }
#else
enum { g_skip = 0 };   // the shipped library cannot leave launches out
#endif
// in-network timing (q4_bench_in_network): launches of the class whose bit is in g_time_mask carry dispatch timestamps
static int g_time_mask = 0;
static std::vector<hipEvent_t>* g_time_events = nullptr;
static std::vector<int>* g_time_bits = nullptr;
static inline void arm_timing(int bit) {
    g_ev_start = g_ev_stop = nullptr;
    if (!(g_time_mask & bit) || !g_time_events) return;
    hipEvent_t a = nullptr, b = nullptr;
    if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) return;
    g_time_events->push_back(a);
    g_time_events->push_back(b);
    if (g_time_bits) g_time_bits->push_back(bit);
    g_ev_start = a;
    g_ev_stop = b;
}
#define Q4_UNLESS(bit, call) do { if (!(g_skip & (bit))) { if (g_time_mask) arm_timing(bit); int rc__ = (call); g_ev_start = g_ev_stop = nullptr; if (rc__) return rc__; } } while (0)

#ifdef Q4_PROFILING
// tools/error_growth.py: the residual stream after the attention half and after the FFN half of every layer, [n_layers][2][dim] halves on
// the device (eager launches only: a copy node would be baked into captured graphs)
static q4_half* g_layer_dump = nullptr;
extern "C" void q4_set_layer_dump(void* p) { g_layer_dump = (q4_half*)p; }
#define Q4_LAYER_DUMP(half_) do { if (g_layer_dump) Q4_HIP(hipMemcpyAsync(g_layer_dump + (size_t)(2 * l + (half_)) * dim, x, (size_t)dim * sizeof(q4_half), hipMemcpyDeviceToDevice, g_stream)); } while (0)
#else
#define Q4_LAYER_DUMP(half_) do { } while (0)
#endif

// The launch sequence of a layer, decided in ONE place from the geometry, the model's record (null: a RunState the library did not build -- no table,
// no hand-off words, the five-launch sequence), the bin, the fusion level and the skip mask.
struct NetForms {
    int ao_form;   // the form of the attention -> o-proj launch for this bin (layer_attn.h), -1: none
    bool ao;       // :320-323 as ONE launch where the geometry, the bin and the stream's CUs admit it; the launch in front of it (the fused QKV GEMV) advances its epoch word
    bool fp;       // :326-332 as ONE launch (gemv_ffn_pair.h) where the shapes and the stream admit it; its tag is the same epoch word
    bool fq;       // ... and the next layer's :300-317 with it (fusion level 5): that layer then has no QKV launch of its own
    bool fa;       // ... and THIS layer's :320-323 in front of it (fusion level 6): the whole layer behind its q / k / v is one launch. Only where level 3 would run the
                   // V-slice role (forms 5 / 6, bins <= 256), whose arithmetic the launch's first phase repeats
};
static NetForms net_forms(const Config* p, const RunState* s, const Model* m, int seq_len_bin) {
    const int dim = p->dim, hidden_dim = p->hidden_dim, head_size = dim / p->n_heads, kv_dim = (p->dim * p->n_kv_heads) / p->n_heads;
    const bool sync = m && m->sync;
    NetForms f;
    const bool kv8 = m && m->kv_format == Q4_KV_FP8;   // FP8 cache: QKV into the staging rows, launch_attention_kv8, o-proj; the FFN half as the level chooses, without fq / fa
    f.ao_form = g_fusion >= 3 && sync && !kv8 ? attention_oproj_form(dim, kv_dim, head_size, p->n_heads, seq_len_bin, s->att != nullptr, att_buffer_bytes(p), g_att_split_min, g_att_chunk) : -1;
    f.ao = f.ao_form >= 0;
    f.fp = g_fusion >= 4 && sync && ffn_pair_covers(dim, hidden_dim);
    f.fq = f.fp && !kv8 && g_fusion >= 5 && ffn_qkv_covers(dim, hidden_dim, kv_dim, head_size, m->rope_table != nullptr);
    f.fa = f.fq && g_fusion >= 6 && (f.ao_form == 5 || f.ao_form == 6) && layer_att_covers(dim, hidden_dim, kv_dim, p->n_heads, seq_len_bin) && !(g_skip & 15);
    return f;
}

extern "C" int q4_run_llama_network(const int* pPos, const Config* p, RunState* s, const TransformerWeights* w, int seq_len_bin) {
    return run_network(pPos, p, s, w, seq_len_bin, false);
}
int q4::run_network(const int* pPos, const Config* p, RunState* s, const TransformerWeights* w, int seq_len_bin, bool have_embedding, bool screened) {
    q4_half* x = s->x;
    const int dim = p->dim;
    const int hidden_dim = p->hidden_dim;
    const int head_size = dim / p->n_heads;
    const int kv_dim = (p->dim * p->n_kv_heads) / p->n_heads;
    const int kv_mul = p->n_heads / p->n_kv_heads;
    const Model* m = model_of(s);
    const float2* rope_table = m ? m->rope_table : nullptr;
    const bool scaled = m && m->rope.kind != Q4_ROPE_NONE;     // RoPE scaling: every rotation from the model's table (level 0: from its frequencies), never from rope_theta
    if (scaled && (!rope_table || !m->inv_freq_dev)) return Q4_ERR_ARG;
    unsigned* sync = m ? m->sync : nullptr;
    const bool kv8 = m && m->kv_format == Q4_KV_FP8;
    uint8_t* const k8 = (uint8_t*)s->key_cache;     // (FP8 models: the caches are bytes)
    uint8_t* const v8 = (uint8_t*)s->value_cache;

    if (!have_embedding)
        Q4_UNLESS(64, q4_copy_embedding(x, w->token_embedding_table, dim, s->shared_data->tokens, pPos));   // :294

    const size_t att_bytes = att_buffer_bytes(p);
    const NetForms f = net_forms(p, s, m, seq_len_bin);
    bool qkv_done = false;                             // the previous launch has left q and the K / V rows of this layer

    for (int l = 0; l < p->n_layers; l++) {
        const PerLayerWeight* L = &w->layers[l];
        // :303. 64-bit: the reference's int overflows at e.g. 13B x 16384 positions (40 * 16384 * 5120 > 2^31); the
        // int-typed entry points of the 1:1 path get pre-offset cache pointers and loff = 0 instead
        const long long loff = (long long)l * p->seq_len * kv_dim;
        if (qkv_done) {
            qkv_done = false;
        } else if (kv8) {
            // ... at EVERY fusion level (the same bits as the 1:1 chain), this position's K / V left in the fp16 staging rows: the attention launch appends them
            Q4_UNLESS(1, launch_qkv_fused(s->q, m->k_row, m->v_row, x, L->rms_att_weight, &L->wq_q, &L->wq_k, &L->wq_v,
                                          dim, kv_dim, 0, pPos, head_size, p->rope_theta, rope_table, f.fp ? sync + SYNC_EPOCH : nullptr, true));
        } else if (g_fusion) {
            // rmsnorm (:300) + qkv (:307, or the three GEMVs of the GQA branch :310-312) + RoPE (:317) in one launch
            Q4_UNLESS(1, launch_qkv_fused(s->q, s->key_cache, s->value_cache, x, L->rms_att_weight, &L->wq_q, &L->wq_k, &L->wq_v,
                                          dim, kv_dim, loff, pPos, head_size, p->rope_theta, rope_table, (f.ao || f.fp) ? sync + SYNC_EPOCH : nullptr));
        } else {
            Q4_TRY(q4_rmsnorm(s->xb, x, L->rms_att_weight, dim));                                      // :300
            if (dim == kv_dim) {
                Q4_TRY(q4_qkv_matvec(s->q, s->key_cache + loff, s->value_cache + loff, s->xb, &L->wq_q, &L->wq_k, &L->wq_v, dim, dim, 0, pPos));
            } else {
                Q4_TRY(q4_matmul_q4(s->q, s->xb, &L->wq_q, dim, dim, 0, -1, nullptr));                 // :310-312
                Q4_TRY(q4_matmul_q4(s->key_cache + loff, s->xb, &L->wq_k, dim, kv_dim, 0, 0, pPos));
                Q4_TRY(q4_matmul_q4(s->value_cache + loff, s->xb, &L->wq_v, dim, kv_dim, 0, 0, pPos));
            }
            if (scaled) Q4_TRY(q4_rope_rotation_freqs(s->q, s->key_cache + loff, p->n_heads, p->n_kv_heads, head_size, pPos, 0, m->inv_freq_dev));
            else Q4_TRY(q4_rope_rotation(s->q, s->key_cache + loff, p->n_heads, p->n_kv_heads, head_size, pPos, 0, p->rope_theta));   // :317
        }
        if (kv8) {
            const size_t eoff = (size_t)l * p->n_kv_heads * p->seq_len;
            Q4_UNLESS(2, launch_attention_kv8(s->xb, s->q, k8 + loff, v8 + loff, m->k_exp + eoff, m->v_exp + eoff, m->k_row, m->v_row, p->n_heads, head_size, kv_mul,
                                              seq_len_bin, p->seq_len, pPos, (float*)s->att, att_bytes, sync && p->n_heads <= SYNC_MAX_HEADS ? sync + SYNC_ARRIVE : nullptr));
            Q4_UNLESS(4, q4_matmul_q4(s->x, s->xb, &L->wq_o, dim, dim, 1, -1, nullptr));
        } else if (f.fa) {
            // (phases A and O of the launch below)
        } else if (f.ao) {
            Q4_UNLESS(6, launch_attention_oproj(x, s->xb, s->q, s->key_cache + loff, s->value_cache + loff, &L->wq_o, dim, kv_dim, p->n_heads,
                                                pPos, seq_len_bin, sync, (float*)s->att, att_bytes, g_att_split_min, g_att_chunk, m->kv_price));
        } else {
        Q4_UNLESS(2, launch_attention(s->xb, s->q, s->key_cache + loff, s->value_cache + loff, p->n_heads, head_size, kv_mul,
                                      seq_len_bin, pPos, (float*)s->att,
                                      att_bytes, sync && p->n_heads <= SYNC_MAX_HEADS ? sync + SYNC_ARRIVE : nullptr));   // :320
        Q4_UNLESS(4, q4_matmul_q4(s->x, s->xb, &L->wq_o, dim, dim, 1, -1, nullptr));                   // :323
        }
        Q4_LAYER_DUMP(0);
        if (f.fp) {
            FfnQkvNext nx = {};
            const bool with_next = f.fq && l + 1 < p->n_layers && !(g_skip & 9);
            if (with_next) {
                const PerLayerWeight* N = &w->layers[l + 1];
                const long long noff = (long long)(l + 1) * p->seq_len * kv_dim;
                nx = FfnQkvNext{N->rms_att_weight, &N->wq_q, &N->wq_k, &N->wq_v, s->q, s->key_cache + noff, s->value_cache + noff, pPos, rope_table,
                                sync + SYNC_EPOCH, kv_dim, head_size};
            }
            const FfnLayerAtt la = {s->xb, s->q, s->key_cache + loff, s->value_cache + loff, &L->wq_o, pPos, p->n_heads, kv_dim, seq_len_bin};
            Q4_UNLESS(8, launch_ffn_pair(x, s->hb, L->rms_ffn_weight, &L->wq_gate, &L->wq_up, &L->wq_down, dim, hidden_dim, sync, ffn_pair_sync_offset(dim), 0u,
                                         with_next ? &nx : nullptr, f.fa ? &la : nullptr));   // :326-332 (+ the next layer's :300-317, + this layer's :320-323)
            qkv_done = with_next;
            Q4_LAYER_DUMP(1);
            continue;
        }
        if (g_fusion) {
            Q4_UNLESS(8, launch_ffn_fused(s->hb, x, L->rms_ffn_weight, &L->wq_gate, &L->wq_up, dim, hidden_dim));   // :326 + :329
        } else {
            Q4_TRY(q4_rmsnorm(s->xb, x, L->rms_ffn_weight, dim));                                      // :326
            Q4_TRY(q4_ffn_matvec_silu(s->hb, s->xb, &L->wq_gate, &L->wq_up, dim, hidden_dim));         // :329
        }
        Q4_UNLESS(16, q4_matmul_q4(s->x, s->hb, &L->wq_down, hidden_dim, dim, 1, -1, nullptr));        // :332
        Q4_LAYER_DUMP(1);
    }
    if (screened) {           // a greedy generating step whose logits nobody reads (q4_step.hip decides): int8 screen + exact refinement of the candidate rows
        if (!m || !m->screen.base) return Q4_ERR_ARG;
        Q4_UNLESS(32, launch_cls_screen(m->screen, s->logits, x, w->rms_final_weight, w->wcls));
    } else if (g_fusion >= 1) {      // one launch where the classifier runs as strips (gemv_strip_cls.h): the final norm inside its x staging
        Q4_UNLESS(32, classifier_with_final_norm(s->logits, x, w->rms_final_weight, w->wcls, p->dim, p->vocab_size));
    } else {
        Q4_UNLESS(32, q4_rmsnorm(x, x, w->rms_final_weight, dim));                                         // :336
        Q4_UNLESS(32, q4_matmul_f16(s->logits, x, w->wcls, p->dim, p->vocab_size, 1, 0, 0, 0, -1, 1.0f));  // :339
    }
    return Q4_OK;
}

// Average duration of one launch class INSIDE the eager decode network (x produced by the previous kernel, caches
// in the state the real token loop leaves them): `tokens` decode steps from the current position with dispatch
// timestamps on the launches of time_mask | report_mask (1 qkv, 2 attention, 4 o-proj, 8 gate/up, 16 down, 32 final
// norm + classifier, 64 embedding); the statistics cover report_mask. The launches are the product's own, only
// hipExtLaunchKernelGGL carries the events.
extern "C" double q4_bench_in_network(int time_mask, int report_mask, const Config* p, RunState* s, const TransformerWeights* w,
                                      int tokens, double* min_us, double* max_us, int* launches) {
    if (!p || !s || !w || tokens < 1 || !g_stream) return -1.0;
    std::vector<hipEvent_t> ev;
    std::vector<int> bits;
    int rc = 0;
    const int pos0 = s->shared_data->pos;
    for (int t = 0; t < tokens && !rc; t++) {
        const int pos = pos0 + t;
        if (pos + 1 >= p->seq_len) break;
        g_time_events = &ev;
        g_time_bits = &bits;
        g_time_mask = time_mask | report_mask;
        rc = q4_run_llama_network(s->pos, p, s, w, pos + 1);
        g_time_mask = 0;
        g_time_events = nullptr;
        g_time_bits = nullptr;
        if (!rc) rc = q4_argmax(s->logits, p->vocab_size, &(s->shared_data->tokens[0]), &(s->shared_data->pos), s->pos, 1);
    }
    if (!rc && hipStreamSynchronize(g_stream) != hipSuccess) rc = Q4_ERR_HIP;
    double total = 0, mn = 1e30, mx = 0;
    int n = 0;
    for (size_t i = 0; i < bits.size() && !rc; i++) {
        if (!(bits[i] & report_mask)) continue;
        float ms = 0;
        if (hipEventElapsedTime(&ms, ev[2 * i], ev[2 * i + 1]) != hipSuccess) { rc = Q4_ERR_HIP; break; }
        const double us = ms * 1000.0;
        total += us;
        n++;
        if (us < mn) mn = us;
        if (us > mx) mx = us;
    }
    for (auto& e : ev) hipEventDestroy(e);
    if (rc || n == 0) return -1.0;
    if (min_us) *min_us = mn;
    if (max_us) *max_us = mx;
    if (launches) *launches = n;
    return total / n;
}
