// q4_sequence.hip -- between the steps of a model: the hand-off state and the fusion level's probation after a timed-out in-launch wait, where a sequence
// begins or resumes, the wait for a published position, context shift. Mirrors llama2_q4.cu:461-463 (generate's reset); the rest is not in the reference.
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "q4_model.h"
#include "option_text.h"
using namespace q4;

static int g_rearm_after = 0;          // > 0: sequences left at fusion level 1 before the level in force is tried again (after a timed-out hand-off)
static int g_rearm_level = 5;          // the fusion level that comes back when the probation ends
static int g_rearm_backoff = 16;       // sequences to sit out after the next time-out: doubles every time, so a box that keeps stalling settles at level 1
static int g_handoff_timeouts = 0;     // timed-out in-launch waits seen by q4_handoff_status since the library was loaded

// Hand-off state between sequences / launch-sequence changes / after a time-out. The EPOCH word is never rewound: the tag of a
// launch is the epoch as it finds it, and the tagged words that outlive a launch -- the attention granules and the split-context
// records in RunState::att -- validate themselves by tag alone, so a tag must never repeat during the life of the model (a second
// sequence that reached the same (position, layer) used to re-create the first one's tag and could merge its stale records).
// Cleared: arrival counters and granules, and the error word when asked. Past 2^31 launches (days of decoding) the epoch does
// start over, together with every buffer that holds tags.
static int clear_handoff_state(const RunState* s, const Model* m, bool error_too) {
    if (!m || !m->sync || m->sync_words <= SYNC_EPOCH + 1) return Q4_OK;
    unsigned* sync = m->sync;
    if (error_too) Q4_HIP(hipMemsetAsync(sync + SYNC_ERROR, 0, sizeof(unsigned), g_stream));
    Q4_HIP(hipMemsetAsync(sync + SYNC_EPOCH + 1, 0, (m->sync_words - SYNC_EPOCH - 1) * sizeof(unsigned), g_stream));
    Q4_HIP(hipStreamSynchronize(g_stream));
    unsigned epoch = 0;
    Q4_HIP(hipMemcpy(&epoch, sync + SYNC_EPOCH, sizeof(epoch), hipMemcpyDeviceToHost));
    if (epoch >= 0x80000000u) {
        Q4_HIP(hipMemsetAsync(sync + SYNC_EPOCH, 0, sizeof(unsigned), g_stream));
        if (s->att) Q4_HIP(hipMemsetAsync(s->att, 0, m->att_bytes, g_stream));
        Q4_HIP(hipStreamSynchronize(g_stream));
    }
    return Q4_OK;
}

extern "C" {

// 0: the reference's 1:1 kernel sequence; 1: fused rmsnorm / RoPE / SiLU epilogues (five launches per layer); 3: attention ->
// o-proj as one launch on top of that (default). Level 2 (QKV -> attention -> o-proj as one launch) was measured slower than
// level 1 in round 2 and removed in round 3: the value selects level 1.
void q4_set_fusion(int level) {
    g_fusion = level <= 0 ? 0 : level >= 6 ? 6 : level == 5 ? 5 : level == 4 ? 4 : level == 3 ? 3 : 1;
    g_rearm_after = 0;          // an explicit choice ends the probation after a time-out (and is the documented way to re-arm at once)
    q4_reset_graphs();
    if (g_stream)
        for (auto& kv : models()) (void)clear_handoff_state(kv.first, &kv.second, false);   // no stale counters / granules across a change of launch sequence
}
int q4_get_fusion(void) { return g_fusion; }

// ---------------------------------------------------------------------------------------------------
// What q4_reset_sequence and q4_resume_sequence share: the position (the device's and SharedData::pos) becomes start_pos, the probation after a
// time-out counts the sequence, the guide ring goes to NONE, the hand-off counters and granules are cleared, the ring receives the tokens.
static int begin_sequence(RunState* s, const int* tokens, int num_tokens, int start_pos) {
    if (start_pos == 0) Q4_HIP(hipMemsetAsync(s->pos, 0, sizeof(int), g_stream));                     // llama2_q4.cu:461
    else Q4_HIP(hipMemcpyAsync(s->pos, &start_pos, sizeof(int), hipMemcpyHostToDevice, g_stream));   // (pageable: staged before the call returns)
    if (g_rearm_after > 0 && --g_rearm_after == 0 && g_fusion == 1) { g_fusion = g_rearm_level; q4_reset_graphs(); }   // probation over
    Model* m = model_of(s);
    if (m && m->guide) Q4_TRY(guide_clear_ring(m));        // a new sequence starts at the guide's state 0
    if (m) Q4_TRY(adaptive_clear_ring(m));                 // ... and a Mirostat span at 2 * tau
    Q4_TRY(clear_handoff_state(s, m, false));     // counters and granules; the error word [0] stays until q4_handoff_status reads it
    Q4_HIP(hipStreamSynchronize(g_stream));
    if (m && start_pos == 0) { m->rows_suspect = false; m->shifted_keep = -1; }   // every row the sequence reads is written again
    s->shared_data->pos = start_pos;                                               // :462
    if (tokens && num_tokens > 0)
        memcpy((void*)s->shared_data->tokens, tokens, sizeof(int) * num_tokens);   // :463
    return Q4_OK;
}
int q4_reset_sequence(RunState* s, const int* prompt_tokens, int num_prompt_tokens) {
    return begin_sequence(s, prompt_tokens, num_prompt_tokens, 0);
}
// q4_reset_sequence that starts at start_pos: the K / V rows below it stay (the caller's contract: they were computed from tokens[0 .. start_pos)).
int q4_resume_sequence(RunState* s, const int* tokens, int num_tokens, int start_pos) {
    if (!s || !s->pos || !s->shared_data || !tokens || num_tokens < 1 || num_tokens > Q4_MAX_SEQ_LEN || start_pos < 0 || start_pos > num_tokens - 1) return Q4_ERR_ARG;
    if (model_of(s) && start_pos > transformer_of(s)->config.seq_len) return Q4_ERR_ARG;
    return begin_sequence(s, tokens, num_tokens, start_pos);
}
// The largest start_pos q4_resume_sequence may be given for `tokens` as the model stands: the common prefix of tokens and the ring, no longer than the
// positions the device has completed, nor than num_tokens - 1 (the last prompt token always runs: it produces the logits).
int q4_common_prefix(const Transformer* t, const int* tokens, int num_tokens) {
    const Model* m = t ? model_of(&t->state) : nullptr;
    if (!m || !tokens || num_tokens < 1) return -Q4_ERR_ARG;
    if (hipStreamSynchronize(g_stream) != hipSuccess) { (void)hipGetLastError(); return 0; }
    if (m->rows_suspect) return 0;
    int limit = t->state.shared_data->pos;
    if (limit > num_tokens - 1) limit = num_tokens - 1;
    if (limit > t->config.seq_len) limit = t->config.seq_len;
    if (m->shifted_keep >= 0 && limit > m->shifted_keep) limit = m->shifted_keep;   // q4_shift_context: the rows above were computed with discarded tokens in view
    int n = 0;
    while (n < limit && t->state.shared_data->tokens[n] == tokens[n]) n++;
    return n;
}
int q4_shared_pos(const RunState* s) { return s->shared_data->pos; }

// ---------------------------------------------------------------------------------------------------
// context shift (q4_kv_shift.hip holds the launch; llama2_q4.h the contract). Not in the reference.
// rows [first, first + n) of a small device ring of `width` bytes per row, moved down by D through the host (the call synchronises anyway)
static int shift_ring_rows(void* ring, size_t width, int first, int n, int D) {
    if (!ring || n <= 0 || width == 0) return Q4_OK;
    std::vector<char> host((size_t)n * width);
    Q4_HIP(hipMemcpy(host.data(), (char*)ring + (size_t)first * width, host.size(), hipMemcpyDeviceToHost));
    Q4_HIP(hipMemcpy((char*)ring + (size_t)(first - D) * width, host.data(), host.size(), hipMemcpyHostToDevice));
    return Q4_OK;
}
int q4_shift_context(Transformer* t, int n_pos, int n_keep, int n_discard, int n_ring) {
    Model* m = t ? model_of(&t->state) : nullptr;
    if (!m) return Q4_ERR_ARG;
    Q4_HIP(hipStreamSynchronize(g_stream));
    const Config* p = &t->config;
    RunState* s = &t->state;
    const int done = s->shared_data->pos;
    if (m->rows_suspect || n_keep < 0 || n_discard < 1 || (long long)n_keep + n_discard > n_pos || n_pos > done || n_pos > p->seq_len ||
        n_ring < n_pos + 1 || n_ring > Q4_MAX_SEQ_LEN)
        return Q4_ERR_ARG;
    const int head_size = p->dim / p->n_heads, D = n_discard, first = n_keep + D, M = n_pos - first;
    if (M > 0) {
        if (!m->rope_table) {
            snprintf(g_last_error, sizeof(g_last_error), "q4_shift_context: the model has no rotation table");
            return Q4_ERR_UNSUPPORTED_SIZE;
        }
        Q4_TRY(launch_kv_shift(s->key_cache, s->value_cache, m->k_exp, m->v_exp, m->kv_format, p->n_layers, p->seq_len, p->n_kv_heads, head_size, n_pos,
                               n_keep, D, (const float*)(m->rope_table + (size_t)D * (head_size / 2))));
    }
    const int new_pos = n_pos - D;
    Q4_HIP(hipMemcpyAsync(s->pos, &new_pos, sizeof(int), hipMemcpyHostToDevice, g_stream));
    Q4_HIP(hipStreamSynchronize(g_stream));
    if (m->guide && m->guide_state) {
        int last = Q4_GUIDE_NONE;
        Q4_HIP(hipMemcpy(&last, m->guide_state + n_pos - 1, sizeof(int), hipMemcpyDeviceToHost));
        Q4_TRY(shift_ring_rows(m->guide_state, sizeof(int), first, M, D));
        if (new_pos >= 1) Q4_HIP(hipMemcpy(m->guide_state + new_pos - 1, &last, sizeof(int), hipMemcpyHostToDevice));   // (M > 0: the moved entry already)
    }
    Q4_TRY(adaptive_shift(m, p->vocab_size, n_pos, first, M, D));
    if (m->logprobs_k >= 0) {
        const size_t K = (size_t)m->logprobs_k;
        Q4_TRY(shift_ring_rows(m->lp_lse, sizeof(float), first, M, D));
        Q4_TRY(shift_ring_rows(m->lp_token, sizeof(float), first, M, D));
        Q4_TRY(shift_ring_rows(m->lp_ids, K * sizeof(int), first, M, D));
        Q4_TRY(shift_ring_rows(m->lp_top, K * sizeof(float), first, M, D));
    }
    Q4_TRY(clear_handoff_state(s, m, false));     // as after a roll-back: counters and granules; the error word stays for q4_handoff_status
    Q4_HIP(hipStreamSynchronize(g_stream));
    int* ring = (int*)s->shared_data->tokens;
    memmove(ring + n_keep, ring + first, (size_t)(n_ring - first) * sizeof(int));
    s->shared_data->pos = new_pos;
    if (m->shifted_keep < 0 || n_keep < m->shifted_keep) m->shifted_keep = n_keep;
    return Q4_OK;
}
int q4_set_context_shift(Transformer* t, int n_keep, int n_discard) {
    Model* m = t ? model_of(&t->state) : nullptr;
    if (!m || n_keep < 0 || n_discard < 0 || (long long)n_keep + n_discard > t->config.seq_len) return Q4_ERR_ARG;
    m->shift_keep = n_keep;
    m->shift_discard = n_discard;
    return Q4_OK;
}
int q4_get_context_shift(const Transformer* t, int* n_keep, int* n_discard) {
    const Model* m = t ? model_of(&t->state) : nullptr;
    if (!m) return Q4_ERR_ARG;
    if (n_keep) *n_keep = m->shift_keep;
    if (n_discard) *n_discard = m->shift_discard;
    return Q4_OK;
}
int q4_parse_context_shift(const char* text, int* n_keep, int* n_discard) {
    if (!text || !n_keep || !n_discard) return Q4_ERR_ARG;
    long keep = 0, discard = 0;
    const char* p = text;
    while (*p) {
        char key[OPTION_KEY_CAP], val[32];
        if (!next_option(&p, key, val, sizeof(val))) return Q4_ERR_ARG;
        long* dst = !strcmp(key, "keep") ? &keep : !strcmp(key, "discard") ? &discard : nullptr;
        if (!dst || val[0] < '0' || val[0] > '9') return Q4_ERR_ARG;          // (no sign, no leading blank)
        char* rest = nullptr;
        *dst = strtol(val, &rest, 10);
        if (*rest || *dst > Q4_MAX_SEQ_LEN) return Q4_ERR_ARG;
    }
    if (discard < 1) return Q4_ERR_ARG;                        // off is the absence of a setting, not a text
    *n_keep = (int)keep;
    *n_discard = (int)discard;
    return Q4_OK;
}
int q4_get_rope_row(const Transformer* t, int pos, float* cos_sin) {
    const Model* m = t ? model_of(&t->state) : nullptr;
    if (!m || !m->rope_table || !cos_sin || pos < 0 || pos >= t->config.seq_len) return Q4_ERR_ARG;
    Q4_HIP(hipStreamSynchronize(g_stream));
    const size_t hp = (size_t)(t->config.dim / t->config.n_heads) / 2;
    Q4_HIP(hipMemcpy(cos_sin, m->rope_table + (size_t)pos * hp, hp * sizeof(float2), hipMemcpyDeviceToHost));
    return Q4_OK;
}

// The in-launch hand-offs of fusion levels 3 and 4 (attention -> o-proj, layer_attn.h; the FFN pair launch, gemv_ffn_pair.h) spin for a bounded time; a spin that ran out
// sets the model's error word: everything computed since is invalid. Synchronises the stream and reports it ONCE: the word,
// the counters and the granules are cleared (the epoch keeps counting: tags never repeat), and the library drops to fusion
// level 1 (no in-launch waits), so the caller can simply redo the sequence -- the token loops of this library do exactly that.
// The level in force comes back by itself after 16 sequences (q4_reset_sequence counts them; 32, 64, ... after further time-outs) or at
// once with q4_set_fusion(level).
int q4_handoff_status(const RunState* s) {
    Q4_HIP(hipStreamSynchronize(g_stream));
    Model* m = model_of(s);
    if (!m || !m->sync) return Q4_OK;
    unsigned flag = 0;
    Q4_HIP(hipMemcpy(&flag, m->sync + SYNC_ERROR, sizeof(flag), hipMemcpyDeviceToHost));
    if (flag) {
        m->rows_suspect = true;     // until the next q4_reset_sequence: nothing computed since the time-out may be kept (q4_common_prefix)
        Q4_TRY(clear_handoff_state(s, m, true));
        g_handoff_timeouts++;
        if (g_fusion >= 3) {    // one transient stall (a profiler attaching, a co-tenant) must not cost every later sequence its 3 %
            g_rearm_level = g_fusion;
            g_fusion = 1;
            g_rearm_after = g_rearm_backoff;
            if (g_rearm_backoff < (1 << 20)) g_rearm_backoff *= 2;
            q4_reset_graphs();
        }
        snprintf(g_last_error, sizeof(g_last_error), "an in-launch hand-off timed out (fusion level %d); state cleared, continuing at fusion level 1 for the next %d sequences", g_rearm_level, g_rearm_after);
        if (!g_quiet) fprintf(stderr, "llama2_q4: %s\n", g_last_error);
        return Q4_ERR_HIP;
    }
    return Q4_OK;
}
int q4_handoff_timeouts(void) { return g_handoff_timeouts; }
// Wait until the device has published position >= pos (argmax_kernel / sample_scan_kernel write the token, fence, then
// SharedData::pos -- "unblocks the CPU", gpu_kernels.h:490). Spins on the pinned word; falls back to the stream state
// so that a failed launch cannot hang the host.
int q4_wait_pos(const RunState* s, int pos) {
    volatile int* p = &s->shared_data->pos;
    for (unsigned spins = 1;; spins++) {
        if (*p >= pos) return Q4_OK;
        if ((spins & 0x3fff) == 0) {
            hipError_t e = hipStreamQuery(g_stream);
            if (e == hipSuccess) return *p >= pos ? Q4_OK : Q4_ERR_ARG;           // stream drained: pos is final
            if (e != hipErrorNotReady) Q4_HIP(e);
        }
        __builtin_ia32_pause();
    }
}
int q4_shared_token(const RunState* s, int index) { return s->shared_data->tokens[index]; }

}  // extern "C"
