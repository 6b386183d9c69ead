// q4_step.hip -- one decode step and the loops over it: per-model graph sets and q4_run_transformer*, the sampler's host side, the hand-off
// state between sequences, the one generate loop (q4_token_loop, q4_loop.h: q4_generate_ids and q4_host.cpp's q4_generate), perplexity and scoring on token ids.
// Mirrors llama2_q4.cu:342-395 (run_transformer), :436-492 (generate), sampler.h, perplexity.h:57-97.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include <stddef.h>
#include <vector>
#include "q4_model.h"
#include "q4_loop.h"
#include "prompt_pass.h"
#include "spec_verify.h"
#include "option_text.h"

namespace q4 {

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

// The logit stages of a generating step, in launch order (q4_model.h LogitStage). Stage i is variant bit STAGE_BIT0 + i.
static const LogitStage* const STAGES[] = {&guide_stage, &dry_stage, &controls_stage, &adaptive_stage};
enum { N_STAGES = sizeof(STAGES) / sizeof(STAGES[0]), STAGE_BIT0 = 6, N_VARIANTS = 1 << (STAGE_BIT0 + N_STAGES) };
static inline int stage_bit(int i) { return 1 << (STAGE_BIT0 + i); }

// graphs: [bin][variant]; variant bit0 = gen_token, bit1 = copyLogits, bit2 = sampled (the sampler launch, its temperature / top-p / coin ring baked in),
// bit3 = Q4_MULTI_STEPS steps per graph, bit4 = the log-probability record launch of q4_set_logprobs (its K and ring baked in), bit5 = the classifier as screen + refine (cls_screen.h),
// from bit6 on one bit per logit stage: its launch, with the address of its parameter block baked in and none of the block's values (the adaptive
// truncation's also holds the addresses of the model's rings). A captured graph holds one model's pointers, so the sets are kept PER MODEL (its RunState): a host that alternates
// a few models on one GPU replays each one's graphs (llama2_q4.cu:342-344 keeps one set for its one model); beyond GRAPH_OWNERS live models the least
// recently used set is dropped and captured again on its next turn (q4_graph_captures counts: a host can see it happen). A set remembers the Config and the
// weights it was captured with: a caller who reuses a RunState with others gets new captures, not a replay of stale pointers.
enum { GRAPH_OWNERS = 4 };
struct GraphSet {
    const RunState* owner;
    const Config* config;
    const TransformerWeights* weights;
    unsigned long long used;
    hipGraphExec_t exec[Q4_MAX_GRAPHS][N_VARIANTS];
    bool captured[Q4_MAX_GRAPHS][N_VARIANTS];
    const Sampler* sampler;            // what the set's sampled graphs have baked in
    float temperature, topp;
    const float* coins;
    const void* block[N_STAGES];       // the parameter block the set's graphs with stage i's launch read
};
static GraphSet g_sets[GRAPH_OWNERS];
static unsigned long long g_set_clock = 0;
static int g_graph_captures = 0;
// a graph is destroyed only after the launch stream has drained -- a replay may still be in flight (eviction and free are rare: the token loop never waits here)
// mask: 0 drops every variant and gives the set up; else the variants with any of the mask's bits -- 4 the sampled ones (what they have baked in is
// forgotten), 16 those with the record launch, stage_bit(i) those with stage i's launch (its block is forgotten)
static void drop_graphs(GraphSet& gs, int mask) {
    bool drained = false;
    for (int i = 0; i < Q4_MAX_GRAPHS; i++)
        for (int v = 0; v < N_VARIANTS; v++)
            if (gs.captured[i][v] && (!mask || (v & mask))) {
                if (!drained) { (void)hipStreamSynchronize(g_stream); drained = true; }
                hipGraphExecDestroy(gs.exec[i][v]);
                gs.captured[i][v] = false;
            }
    if (!mask) gs.owner = nullptr;
    if (!mask || (mask & 4)) { gs.sampler = nullptr; gs.coins = nullptr; }
    for (int i = 0; i < N_STAGES; i++)
        if (!mask || (mask & stage_bit(i))) gs.block[i] = nullptr;
}
void drop_graphs_of(const RunState* s) {
    for (GraphSet& gs : g_sets)
        if (gs.owner == s) drop_graphs(gs, 0);
}
void drop_logprob_graphs_of(const RunState* s) {
    for (GraphSet& gs : g_sets)
        if (gs.owner == s) drop_graphs(gs, 16);
}
static GraphSet& graph_set_of(const RunState* owner, const Config* p, const TransformerWeights* w) {
    GraphSet* pick = nullptr;
    for (GraphSet& gs : g_sets)
        if (gs.owner == owner) { pick = &gs; break; }
    if (pick && (pick->config != p || pick->weights != w)) drop_graphs(*pick, 0);   // the same RunState with another Config or other weights
    if (!pick || !pick->owner) {
        for (GraphSet& gs : g_sets)
            if (!pick || (gs.owner == nullptr && pick->owner != nullptr) || (((gs.owner == nullptr) == (pick->owner == nullptr)) && gs.used < pick->used)) pick = &gs;
        if (pick->owner) drop_graphs(*pick, 0);
        pick->owner = owner; pick->config = p; pick->weights = w;
    }
    pick->used = ++g_set_clock;
    return *pick;
}

// A step runs its classifier as screen + refine only when nothing but the greedy token is taken from its logits: a greedy generating step of a token
// loop (may_screen: the public per-step entry points never pass it -- their callers read RunState::logits), no fp32 copy, no log-probability records, a
// model with a screening copy whose shape the launch stream still admits, the fused sequence, the switch on and no logit stage (their launches rewrite
// whole logits).
static bool any_stage_on(const Sampler* sampler, const Model* m) {
    for (const LogitStage* st : STAGES)
        if (st->on(sampler, m)) return true;
    return false;
}
static bool step_screens(const Model* m, bool may_screen, int gen_token, bool greedy, int copyLogits, const Sampler* sampler) {
    return may_screen && g_greedy_screen && gen_token && greedy && !copyLogits && g_fusion >= 1 && m && m->logprobs_k < 0 && m->screen.base &&
           !any_stage_on(sampler, m) && cls_screen_shape(m->screen.n, m->screen.d);
}

// The graph bin of a step whose sequence length is seq_len (llama2_q4.cu:355-360): the index of its graph set and the bin's size
static int graph_bin(int seq_len, const Config* p, int* seq_len_bin_out) {
    int graphIndex;
    int seq_len_bin = 128;
    for (graphIndex = 0; graphIndex < Q4_MAX_GRAPHS - 1; seq_len_bin *= 2, graphIndex++)
        if (seq_len <= seq_len_bin) break;                                         // :356-359
    if ((seq_len > seq_len_bin) || (graphIndex == Q4_MAX_GRAPHS - 1)) seq_len_bin = p->seq_len;   // :360
    *seq_len_bin_out = seq_len_bin;
    return graphIndex;
}

// ---- what a pass (prompt pass, verify pass) may touch: the admission's position rules, in one place ----
// q4_set_pass_context: the exclusive upper bound on the positions of a pass; in force for a model: min(value, seq_len). 256 (the default, and the
// least) keeps passes to the V-slice bins.
static int g_pass_context = PASS_CONTEXT_MIN;
static int pass_bound(const Config* p) { return g_pass_context < p->seq_len ? g_pass_context : p->seq_len; }
// The seq_len_bin argument the step at position `pos` hands to run_network (run_transformer_steps_screenable): the graph bin of pos + 1 where steps run
// by bin (graphs, eager bins), pos + 1 itself without graphs.
static int step_bin_arg(const Config* p, int pos) {
    int bin;
    (void)graph_bin(pos + 1, p, &bin);
    return g_use_graphs ? bin : pos + 1;
}
// Where the bin of `pos` ends: positions [0, 256) are one stretch for a pass (the V-slice forms of bins 128 and 256), then [256, 512), [512, 1024), ...
// No pass reaches across an end: above 255 the step's attention form or its chunk size may change there.
static int pass_bin_end(int pos) {
    int end = 256;
    while (end <= pos && end < Q4_MAX_SEQ_LEN) end *= 2;
    return end;
}
bool pass_attention_plan(const Config* p, const RunState* s, int pos, int n, PassAttention* out) {
    if (pos < 0 || n < 1 || pos + n > p->seq_len || p->n_heads < 1) return false;
    const int head_size = p->dim / p->n_heads, kv_dim = (p->dim * p->n_kv_heads) / p->n_heads;
    int kind = -1, arg = -1, form = -1;
    for (int i = 0; i < n; i++) {
        const int arg_i = step_bin_arg(p, pos + i);
        if (arg_i != arg) form = attention_oproj_form(p->dim, kv_dim, head_size, p->n_heads, arg_i, s->att != nullptr, att_buffer_bytes(p), g_att_split_min, g_att_chunk);
        const int kind_i = form == 5 || form == 6 ? 5 : form >= 2 && form <= 4 ? form : -1;   // V-slice forms mix (prompt_attention_kernel picks per token); a split form stands alone
        if (kind_i < 0 || (i > 0 && kind_i != kind)) return false;
        if (kind_i != 5 && g_use_graphs && i > 0 && arg_i != arg) return false;               // split tokens of one pass share the step's launch shape
        kind = kind_i;
        arg = arg_i;
    }
    out->form = kind;
    out->chunk = kind == 4 ? 64 : kind == 2 ? 128 : kind == 3 ? 256 : 0;
    out->nsp = kind == 5 ? 0 : divUp(arg, out->chunk);       // (arg: the last position's -- without graphs its own size, the largest of the pass)
    out->nsp_of_bin = g_use_graphs ? out->nsp : 0;
    return true;
}

// A prompt pass (prompt_pass.h) in place of the per-token prompt steps from `pos`: how many positions it takes, 0 for none. Only a token
// loop asks (the per-step entry points, scoring and perplexity keep their steps), and only where the pass computes what the steps would and nothing reads
// what it leaves out: the switch on; the fusion level in force >= 3 with an attention form the pass reproduces at every position it touches
// (pass_attention_plan: the V-slice forms 5 / 6, or one split-context form 4 / 2 / 3) -- so never the level-1 redo after a time-out --; the geometry
// prompt_pass_covers admits (fp16 cache, unmasked stream); every position prompt-only, inside `steps`, below the bound of q4_set_pass_context and inside
// the bin of `pos`; no log-probability records (they describe prompt steps' logits); neither the guide nor the adaptive truncation on (their state by
// position is put to NONE per prompt step); no context-shift offset. (copyLogits: a token loop never asks for it.)
static int g_prompt_ingest = PROMPT_PASS_MAX;
static int g_prompt_passes = 0;
static int prompt_pass_tokens(const Transformer* t, const Model* m, const Sampler* sampler, int pos, int num_prompt_tokens, int steps, int off) {
    if (g_prompt_ingest < 2 || g_fusion < 3 || off != 0 || !m || m->logprobs_k >= 0) return 0;
    const Config* p = &t->config;
    int n = num_prompt_tokens - 1 - pos;
    if (n > g_prompt_ingest) n = g_prompt_ingest;
    if (n > steps - pos) n = steps - pos;
    if (n > pass_bin_end(pos) - pos) n = pass_bin_end(pos) - pos;
    if (n > pass_bound(p) - pos) n = pass_bound(p) - pos;
    if (n < 2 || guide_stage.on(sampler, m) || adaptive_stage.on(sampler, m) || !prompt_pass_covers(p, m)) return 0;
    PassAttention plan;
    return pass_attention_plan(p, &t->state, pos, n, &plan) ? n : 0;
}


// A verify pass (spec_verify.h) at position `pos` with n_draft drafts, positions pos .. pos + n_draft: what a prompt pass requires -- the
// fusion level in force >= 3 with an attention form the pass reproduces at every position (pass_attention_plan), prompt_pass_covers' geometry (fp16 cache,
// unmasked stream), no log-probability records, no guide, no context-shift offset, every position inside the bin of `pos`, below the bound of
// q4_set_pass_context and inside seq_len -- plus a classifier shape the pass's launch
// takes. A token loop adds (sampler non-null): temperature 0 -- or, with the model's spec_sampled switch on, a sampler the row form of the sampling
// launches takes (sample_rows_covers) --, no logit stage on, every position inside `steps`. With all of that off a greedy generating
// step leaves, by position: its K / V rows, ring[pos + 1], the two position words; and, not by position: RunState::logits, RunState::x (un-normalised
// behind the strips classifier; what the pass writes), the scratch vectors xb / hb / q / att (rewritten by every step before it reads them), the hand-off
// epoch (never rewound; a pass does not advance it, as a prompt pass does not), the screen's tallies (q4_screen_candidates counts screened steps: a pass
// screens nothing). Guide states, Mirostat's mu, record rings, the coin ring and logits_array are written only by what the admission excludes.
static bool verify_covers(const Transformer* t, const Model* m, const Sampler* sampler, int pos, int n_draft, int steps, int off) {
    if (g_fusion < 3 || off != 0 || !m || m->logprobs_k >= 0 || m->guide || n_draft < 1 || n_draft > VERIFY_MAX_DRAFT || pos < 0) return false;
    const Config* p = &t->config;
    if (pos + n_draft >= pass_bin_end(pos) || pos + n_draft >= pass_bound(p) || pos + n_draft >= steps) return false;
    if (sampler && sampler->temperature != 0.0f) {
        // q4_set_speculative_sampled: the pass under the sampler -- the row form of its two launches (the on-chip vocabulary, a finite temperature above 0;
        // a negative one keeps the one-block softmax of the step) and a vocabulary that is the model's
        if (!m->spec_sampled || sampler->vocab_size != p->vocab_size || !sample_rows_covers(sampler)) return false;
    }
    if (sampler && any_stage_on(sampler, m)) return false;
    if (!prompt_pass_covers(p, m) || !verify_cls_covers(p->dim, p->vocab_size)) return false;
    PassAttention plan;
    return pass_attention_plan(p, &t->state, pos, n_draft + 1, &plan);
}
// The drafter's answer for ring[0 .. n_tokens), at most max_draft ids, cut in front of the first id outside the vocabulary
static int ask_drafter(const Model* m, const int* ring, int n_tokens, int max_draft, int vocab, int* draft) {
    int n = m->drafter ? m->drafter(m->drafter_ctx, ring, n_tokens, max_draft, draft) : q4_spec_draft(ring, n_tokens, max_draft, m->spec_ngram_max, m->spec_ngram_min, draft);
    if (n > max_draft) n = max_draft;
    for (int i = 0; i < n; i++)
        if (draft[i] < 0 || draft[i] >= vocab) { n = i; break; }
    return n < 0 ? 0 : n;
}

}  // namespace q4

using namespace q4;

extern "C" __attribute__((visibility("hidden"))) int q4_copy_logits_at_pos(float* logits_array, const q4_half* logits, int vocab_size, const int* pPos);

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

// The greedy steps' classifier as an int8 screen + exact refinement (cls_screen.h). 1 (default): on, for models that have a screening copy; 0: off.
void q4_set_greedy_screen(int on) {
    g_greedy_screen = on ? 1 : 0;
    q4_reset_graphs();
}
int q4_get_greedy_screen(void) { return g_greedy_screen; }

// Prompt passes of the token loop (prompt_pass.h): the most positions one pass takes; 0 (and 1) off. No captured graph contains a pass: nothing to drop.
void q4_set_prompt_ingest(int max_tokens) { g_prompt_ingest = max_tokens < 2 ? 0 : max_tokens > PROMPT_PASS_MAX ? PROMPT_PASS_MAX : max_tokens; }
int q4_get_prompt_ingest(void) { return g_prompt_ingest; }
int q4_prompt_passes(void) { return g_prompt_passes; }
// The exclusive upper bound on the positions a prompt pass or a verify pass may touch (process-wide; min(value, seq_len) holds for a model). 256, the
// default and the least value, keeps the passes to the V-slice bins; above it they follow the step into the split-context bins. No captured graph
// contains a pass: nothing to drop.
void q4_set_pass_context(int positions) { g_pass_context = positions > PASS_CONTEXT_MIN ? positions : PASS_CONTEXT_MIN; }
int q4_get_pass_context(void) { return g_pass_context; }

// ---- speculative greedy decoding: the settings, the built-in drafter, the primitive (spec_verify.h) ----
int q4_spec_draft(const int* tokens, int n_tokens, int max_draft, int ngram_max, int ngram_min, int* draft_out) {
    if (!tokens || !draft_out || n_tokens < 2 || max_draft < 1 || ngram_min < 1 || ngram_max < ngram_min) return 0;
    for (int g = ngram_max < n_tokens - 1 ? ngram_max : n_tokens - 1; g >= ngram_min; g--) {
        const int* tail = tokens + n_tokens - g;
        for (int j = n_tokens - g - 1; j >= 0; j--) {
            if (memcmp(tokens + j, tail, (size_t)g * sizeof(int)) != 0) continue;
            int n = n_tokens - (j + g);
            if (n > max_draft) n = max_draft;
            memcpy(draft_out, tokens + j + g, (size_t)n * sizeof(int));
            return n;
        }
    }
    return 0;
}
static bool speculative_ok(int max_draft, int ngram_max, int ngram_min) {
    return max_draft == 0 || (max_draft >= 1 && max_draft <= Q4_SPEC_MAX_DRAFT && ngram_min >= 1 && ngram_min <= ngram_max && ngram_max <= Q4_SPEC_MAX_NGRAM);
}
int q4_set_speculative(Transformer* t, int max_draft, int ngram_max, int ngram_min) {
    Model* m = t ? model_of(&t->state) : nullptr;
    if (!m || !speculative_ok(max_draft, ngram_max, ngram_min)) return Q4_ERR_ARG;
    m->spec_draft = max_draft;
    m->spec_ngram_max = max_draft ? ngram_max : 0;
    m->spec_ngram_min = max_draft ? ngram_min : 0;
    return Q4_OK;
}
int q4_get_speculative(const Transformer* t, int* max_draft, int* ngram_max, int* ngram_min) {
    const Model* m = t ? model_of(&t->state) : nullptr;
    if (!m) return Q4_ERR_ARG;
    if (max_draft) *max_draft = m->spec_draft;
    if (ngram_max) *ngram_max = m->spec_ngram_max;
    if (ngram_min) *ngram_min = m->spec_ngram_min;
    return Q4_OK;
}
int q4_parse_speculative(const char* text, int* max_draft, int* ngram_max, int* ngram_min) {
    if (!text || !max_draft || !ngram_max || !ngram_min) return Q4_ERR_ARG;
    long v[3] = {4, 3, -1};               // (min left out: 2, or the longest n-gram where that is shorter)
    const char* p = text;
    while (*p) {
        char key[OPTION_KEY_CAP], val[32];
        if (!next_option(&p, key, val, sizeof(val))) return Q4_ERR_ARG;
        long* dst = !strcmp(key, "draft") ? &v[0] : !strcmp(key, "ngram") ? &v[1] : !strcmp(key, "min") ? &v[2] : nullptr;
        if (!dst || val[0] < '0' || val[0] > '9') return Q4_ERR_ARG;          // (no sign, no leading blank)
        char* rest = nullptr;
        *dst = strtol(val, &rest, 10);
        if (*rest || *dst > 1000) return Q4_ERR_ARG;
    }
    if (v[2] < 0) v[2] = v[1] < 2 ? v[1] : 2;
    if (!speculative_ok((int)v[0], (int)v[1], (int)v[2])) return Q4_ERR_ARG;
    *max_draft = (int)v[0];
    *ngram_max = (int)v[1];
    *ngram_min = (int)v[2];
    return Q4_OK;
}
int q4_parse_speculative_sampled(const char* text, int* on) {     // the CLI's Q4_SPECULATIVE_SAMPLED: "0" or "1", nothing else
    if (!text || !on || (text[0] != '0' && text[0] != '1') || text[1]) return Q4_ERR_ARG;
    *on = text[0] - '0';
    return Q4_OK;
}
int q4_set_drafter(Transformer* t, q4_drafter_fn fn, void* ctx) {
    Model* m = t ? model_of(&t->state) : nullptr;
    if (!m) return Q4_ERR_ARG;
    m->drafter = fn;
    m->drafter_ctx = fn ? ctx : nullptr;
    return Q4_OK;
}
int q4_spec_stats(const Transformer* t, long long* passes, long long* drafted, long long* accepted) {
    const Model* m = t ? model_of(&t->state) : nullptr;
    if (!m) return Q4_ERR_ARG;
    if (passes) *passes = m->spec_passes;
    if (drafted) *drafted = m->spec_drafted;
    if (accepted) *accepted = m->spec_accepted;
    return Q4_OK;
}
int q4_verify_covers(const Transformer* t, int pos, int n_draft) {
    const Model* m = t ? model_of(&t->state) : nullptr;
    return m && verify_covers(t, m, nullptr, pos, n_draft, t->config.seq_len, 0) ? 1 : 0;
}
int q4_verify_tokens(Transformer* t, const int* draft, int n_draft, int* out_tokens, int* n_accepted) {
    Model* m = t ? model_of(&t->state) : nullptr;
    if (!m || !draft || !out_tokens || !n_accepted || n_draft < 1 || n_draft > Q4_SPEC_MAX_DRAFT) return Q4_ERR_ARG;
    for (int i = 0; i < n_draft; i++)
        if (draft[i] < 0 || draft[i] >= t->config.vocab_size) return Q4_ERR_ARG;
    Q4_HIP(hipStreamSynchronize(g_stream));
    const int pos = t->state.shared_data->pos;
    if (m->rows_suspect || !verify_covers(t, m, nullptr, pos, n_draft, t->config.seq_len, 0)) return Q4_NOT_ADMITTED;
    Q4_TRY(run_verify_pass(&t->config, &t->state, &t->weights, m, pos, draft, n_draft));
    Q4_HIP(hipStreamSynchronize(g_stream));
    const int acc = t->state.shared_data->pos - (pos + 1);
    if (acc < 0 || acc > n_draft) return Q4_ERR_HIP;
    m->spec_passes++;
    m->spec_drafted += n_draft;
    m->spec_accepted += acc;
    for (int i = 0; i <= acc; i++) out_tokens[i] = t->state.shared_data->tokens[pos + 1 + i];
    *n_accepted = acc;
    return Q4_OK;
}
int q4_screen_candidates(const Transformer* t, int* last, int* max, long long* total, long long* steps) {
    const Model* m = t ? model_of(&t->state) : nullptr;
    if (!m) return Q4_ERR_ARG;
    unsigned c[SCREEN_WORDS] = {};
    if (m->screen.base) {
        Q4_HIP(hipStreamSynchronize(g_stream));
        Q4_HIP(hipMemcpy(c, m->screen.count, sizeof(c), hipMemcpyDeviceToHost));
    }
    unsigned long long wide[SCREEN_WORDS / 2];
    memcpy(wide, c, sizeof(c));
    if (c[SCREEN_OPEN]) {     // the last screened step's tally is closed by the next one's screen launch: close it here
        c[SCREEN_LAST] = c[SCREEN_CUR];
        if (c[SCREEN_CUR] > c[SCREEN_MAX]) c[SCREEN_MAX] = c[SCREEN_CUR];
        wide[SCREEN_TOTAL / 2] += c[SCREEN_CUR];
    }
    if (last) *last = (int)c[SCREEN_LAST];
    if (max) *max = (int)c[SCREEN_MAX];
    if (total) *total = (long long)wide[SCREEN_TOTAL / 2];
    if (steps) *steps = (long long)wide[SCREEN_STEPS / 2];
    return Q4_OK;
}

void q4_reset_graphs(void) {
    for (GraphSet& gs : g_sets) drop_graphs(gs, 0);
}
int q4_graph_captures(void) { return g_graph_captures; }

// ---------------------------------------------------------------------------------------------------
// sampler.h
int build_sampler(Sampler* sampler, int vocab_size, float temperature, float topp, unsigned long long rng_seed) {
    memset(sampler, 0, sizeof(*sampler));
    sampler->vocab_size = vocab_size;
    sampler->temperature = temperature;
    sampler->topp = topp;
    sampler->rng_state = rng_seed;
    Q4_HIP(hipMalloc((void**)&sampler->indices, vocab_size * sizeof(int)));        // sampler.h:22
    return Q4_OK;
}
// Coins of the sampled steps that run inside captured graphs: the xorshift stream stays on the host (sampler.h:31-40), the values
// of the steps a replay covers are copied to a device ring indexed by position just before the replay (one small async copy per
// replay), and topp_sample_kernel reads coins[position] -- so the launch needs no per-step argument and sampled steps go out
// eight per replay like greedy ones. (The Sampler struct is the reference's: the ring lives beside it.)
struct CoinRing { float* host; float* dev; int cap; };
static std::map<const Sampler*, CoinRing> g_coin_rings;
static int coin_ring_for(const Sampler* sampler, int positions, CoinRing** out) {
    CoinRing& r = g_coin_rings[sampler];
    if (r.cap < positions) {
        if (r.host) hipHostFree(r.host);
        if (r.dev) hipFree(r.dev);
        r = CoinRing{nullptr, nullptr, 0};
        Q4_HIP(hipHostMalloc((void**)&r.host, (size_t)positions * sizeof(float), hipHostMallocDefault));
        Q4_HIP(hipMalloc((void**)&r.dev, (size_t)positions * sizeof(float)));
        // zeroed on both sides: a caller whose `pos` runs behind the device position (q4_run_transformer_at / _steps with a stale `pos`: the
        // sampled step reads coins[device position], the host fills ring[pos + i]) then samples with coin 0.0 -- the most probable token,
        // deterministic -- instead of with uninitialised memory. INTEGRATION.md: `pos` must equal the device position for sampled steps.
        memset(r.host, 0, (size_t)positions * sizeof(float));
        Q4_HIP(hipMemsetAsync(r.dev, 0, (size_t)positions * sizeof(float), g_stream));
        r.cap = positions;
    }
    *out = &r;
    return Q4_OK;
}
// The coins of a verify pass under the sampler (spec_verify.h) at positions pos .. pos + n_draft: drawn from the sampler's stream into the ring -- the
// coin at a position is the same value whoever draws it -- and the stream put back where it stood. The pass's advance m says how many positions ran, and
// the caller then draws m + 1: one coin per position that ran, as the steps draw them. Entries above the new position are stale and harmless: whatever
// runs there next writes its own.
static int stage_pass_coins(Sampler* sampler, const Config* p, int pos, int n_draft, const float** coins_dev) {
    CoinRing* ring = nullptr;
    Q4_TRY(coin_ring_for(sampler, p->seq_len, &ring));
    if (pos < 0 || pos + n_draft >= ring->cap) return Q4_ERR_ARG;
    const unsigned long long rng = sampler->rng_state;
    for (int i = 0; i <= n_draft; i++) ring->host[pos + i] = random_f32(&sampler->rng_state);
    sampler->rng_state = rng;
    Q4_HIP(hipMemcpyAsync(ring->dev + pos, ring->host + pos, (size_t)(n_draft + 1) * sizeof(float), hipMemcpyHostToDevice, g_stream));
    *coins_dev = ring->dev;
    return Q4_OK;
}
void destroy_sampler(Sampler* sampler) {
    sample_rows_release(sampler);
    for (int i = 0; i < N_STAGES; i++) {
        if (!STAGES[i]->forget) continue;
        if (const void* block = STAGES[i]->block(sampler)) {        // graphs with the stage's launch hold the block's address
            for (GraphSet& gs : g_sets)
                if (gs.block[i] == block) drop_graphs(gs, stage_bit(i));
            if (g_stream) hipStreamSynchronize(g_stream);
        }
        STAGES[i]->forget(sampler);
    }
    auto cr = g_coin_rings.find(sampler);
    if (cr != g_coin_rings.end()) {
        for (GraphSet& gs : g_sets)
            if (gs.sampler == sampler) drop_graphs(gs, 4);
        if (g_stream) hipStreamSynchronize(g_stream);
        if (cr->second.host) hipHostFree(cr->second.host);
        if (cr->second.dev) hipFree(cr->second.dev);
        g_coin_rings.erase(cr);
    }
    if (sampler->indices) hipFree(sampler->indices);
    if (sampler->tempStorage_sort) hipFree(sampler->tempStorage_sort);
    if (sampler->tempStorage_scan) hipFree(sampler->tempStorage_scan);
    memset(sampler, 0, sizeof(*sampler));
}
unsigned int random_u32(unsigned long long* state) {                               // sampler.h:31-37
    *state ^= *state >> 12;
    *state ^= *state << 25;
    *state ^= *state >> 27;
    return (unsigned int)((*state * 0x2545F4914F6CDD1Dull) >> 32);
}
float random_f32(unsigned long long* state) { return (random_u32(state) >> 8) / 16777216.0f; }   // :38-40

Sampler* q4_sampler_new(int vocab_size, float temperature, float topp, unsigned long long rng_seed) {
    Sampler* s = (Sampler*)calloc(1, sizeof(Sampler));
    if (build_sampler(s, vocab_size, temperature, topp, rng_seed)) { free(s); return nullptr; }
    return s;
}
void q4_sampler_delete(Sampler* s) {
    if (!s) return;
    destroy_sampler(s);
    free(s);
}

__attribute__((visibility("hidden"))) int q4_sample_topp_device(Sampler* sampler, RunState* s, float coin, const float* coins, q4_half* x_next,
                                                                const q4_half* table, int dim);   // q4_sampling.hip
__attribute__((visibility("hidden"))) int q4_sample_topp_prepare(Sampler* sampler);

static bool sampler_is_greedy(const Sampler* sampler, int gen_token) {
    return sampler->temperature == 0.0f || !gen_token;                             // sampler.h:47
}

// sample(), sampler.h:43-82. `launch_argmax` false when the captured graph already contains it.
static int sample_impl(Sampler* sampler, RunState* s, int gen_token, bool launch_argmax) {
    float coin = random_f32(&sampler->rng_state);                                  // :45, drawn every step (P8)
    if (sampler_is_greedy(sampler, gen_token)) {
        if (launch_argmax)
            return q4_argmax(s->logits, sampler->vocab_size, &(s->shared_data->tokens[0]), &(s->shared_data->pos), s->pos, gen_token);
        return Q4_OK;
    }
    return q4_sample_topp_device(sampler, s, coin, nullptr, nullptr, nullptr, 0);
}
int q4_sample(Sampler* sampler, RunState* s, int gen_token) { return sample_impl(sampler, s, gen_token, true); }

// What a step runs behind its network: the fp32 copy of the logits, the record launch, the logit stages that are on (block[i] non-null), the argmax or
// the sampler, the record's look-up of the chosen token. ONE list for both paths. captured: inside a capture -- a sampled step's coin comes from
// the ring `coins` by position (the caller draws it), and a step that feeds the next (feed_next) leaves the token's embedding row in s->x. Eager:
// sample_impl draws the step's coin itself.
struct StepTail {
    int gen_token, copyLogits;
    bool greedy, lp_greedy, lp_pick;
    const Model* lpm;                  // null: no record launch
    const Model* model;
    Sampler* sampler;
    const void* block[N_STAGES];
};
static int step_tail(const StepTail& t, const Config* p, RunState* s, const TransformerWeights* w, bool captured, const float* coins, bool feed_next) {
    if (t.copyLogits) Q4_TRY(q4_copy_logits_at_pos(s->logits_array, s->logits, p->vocab_size, s->pos));   // :377-382
    if (t.lpm) Q4_TRY(launch_logprobs_step(t.lpm, p, s, t.gen_token, t.lp_greedy));   // (before the sampler: it advances the position and overwrites the logits;
    for (int i = 0; i < N_STAGES; i++)                                                //  in front of the stages: the records describe the model's raw logits)
        if (t.block[i]) Q4_TRY(STAGES[i]->launch(t.block[i], t.model, p, s));
    if (!captured) Q4_TRY(sample_impl(t.sampler, s, t.gen_token, true));
    else if (!t.greedy)                // sampler.h:51-81 inside the graph
        Q4_TRY(q4_sample_topp_device(t.sampler, s, 0.f, coins, feed_next ? s->x : nullptr, w->token_embedding_table, p->dim));
    else if (feed_next)
        Q4_TRY(launch_argmax_feed(s->logits, p->vocab_size, &(s->shared_data->tokens[0]), &(s->shared_data->pos), s->pos, s->x, w->token_embedding_table, p->dim));
    else
        Q4_TRY(q4_argmax(s->logits, p->vocab_size, &(s->shared_data->tokens[0]), &(s->shared_data->pos), s->pos, t.gen_token));
    return t.lp_pick ? launch_logprobs_pick(t.lpm, p, s) : Q4_OK;
}

// ---- verify passes under the temperature / top-p sampler (spec_verify.h): the switch, the probe, the primitive ----
int q4_set_speculative_sampled(Transformer* t, int on) {
    Model* m = t ? model_of(&t->state) : nullptr;
    if (!m) return Q4_ERR_ARG;
    m->spec_sampled = on != 0;
    return Q4_OK;
}
int q4_get_speculative_sampled(const Transformer* t) {
    const Model* m = t ? model_of(&t->state) : nullptr;
    return m && m->spec_sampled ? 1 : 0;
}
int q4_verify_covers_sampled(const Transformer* t, const Sampler* sampler, int pos, int n_draft) {
    const Model* m = t ? model_of(&t->state) : nullptr;
    return m && sampler && sampler->temperature != 0.0f && verify_covers(t, m, sampler, pos, n_draft, t->config.seq_len, 0) ? 1 : 0;
}
int q4_verify_tokens_sampled(Transformer* t, Sampler* sampler, const int* draft, int n_draft, int* out_tokens, int* n_accepted) {
    Model* m = t ? model_of(&t->state) : nullptr;
    if (!m || !sampler || !draft || !out_tokens || !n_accepted || n_draft < 1 || n_draft > Q4_SPEC_MAX_DRAFT) return Q4_ERR_ARG;
    for (int i = 0; i < n_draft; i++)
        if (draft[i] < 0 || draft[i] >= t->config.vocab_size) return Q4_ERR_ARG;
    Q4_HIP(hipStreamSynchronize(g_stream));
    const int pos = t->state.shared_data->pos;
    if (m->rows_suspect || !q4_verify_covers_sampled(t, sampler, pos, n_draft)) return Q4_NOT_ADMITTED;
    const float* coins = nullptr;
    Q4_TRY(stage_pass_coins(sampler, &t->config, pos, n_draft, &coins));
    Q4_TRY(run_verify_pass(&t->config, &t->state, &t->weights, m, pos, draft, n_draft, sampler, coins));
    Q4_HIP(hipStreamSynchronize(g_stream));
    const int acc = t->state.shared_data->pos - (pos + 1);
    if (acc < 0 || acc > n_draft) return Q4_ERR_HIP;
    for (int i = 0; i <= acc; i++) (void)random_f32(&sampler->rng_state);      // one coin per position that ran
    m->spec_passes++;
    m->spec_drafted += n_draft;
    m->spec_accepted += acc;
    for (int i = 0; i <= acc; i++) out_tokens[i] = t->state.shared_data->tokens[pos + 1 + i];
    *n_accepted = acc;
    return Q4_OK;
}

// ---------------------------------------------------------------------------------------------------
// run_transformer, llama2_q4.cu:346-395
int q4_run_transformer(int gen_token, const Config* p, RunState* s, const TransformerWeights* w, int copyLogits,
                       Sampler* pSampler) {
    return q4_run_transformer_at(s->shared_data->pos, gen_token, p, s, w, copyLogits, pSampler);   // :354
}

// The same step with the position supplied by the caller instead of read back from SharedData::pos: the device keeps
// its own position (`s->pos`) and reads its input token from the ring, so step pos+1 can be queued while step pos is
// still running (generate() below); only the graph bin depends on the host's idea of the position.
int q4_run_transformer_at(int pos, int gen_token, const Config* p, RunState* s, const TransformerWeights* w, int copyLogits,
                          Sampler* pSampler) {
    return q4_run_transformer_steps(pos, 1, gen_token, p, s, w, copyLogits, pSampler);
}

// `nsteps` consecutive greedy steps (positions pos .. pos + nsteps - 1, same gen_token) as ONE graph replay: the device
// advances its own position and feeds itself the tokens (argmax_kernel writes the ring, copy_embedding reads it), so a
// replay needs nothing from the host between steps -- the per-replay launch cost is paid once per nsteps tokens. Only
// nsteps == 1 or Q4_MULTI_STEPS are captured; the caller keeps a group inside one sequence-length bin (q4_steps_that_fit).
int q4_run_transformer_steps(int pos, int nsteps, int gen_token, const Config* p, RunState* s, const TransformerWeights* w,
                             int copyLogits, Sampler* pSampler) {
    return run_transformer_steps_screenable(pos, nsteps, gen_token, p, s, w, copyLogits, pSampler, 0);
}
// ... for the token loops of this library (q4_token_loop below, q4_chat; q4_loop.h): may_screen says that nobody reads the group's logits
int run_transformer_steps_screenable(int pos, int nsteps, int gen_token, const Config* p, RunState* s, const TransformerWeights* w, int copyLogits,
                                     Sampler* pSampler, int may_screen) {
    const int seq_len = pos + nsteps;                                              // :354 (of the group's last step)
    const bool greedy = sampler_is_greedy(pSampler, gen_token);
    int seq_len_bin;
    const int graphIndex = graph_bin(seq_len, p, &seq_len_bin);
    if (nsteps != 1 && (nsteps != g_multi_steps || g_use_graphs != 1)) return Q4_ERR_ARG;
    if (pos < 0 || pos + nsteps > p->seq_len) return Q4_ERR_ARG;
    Model* const mdl = model_of(s);
    const bool screened = step_screens(mdl, may_screen != 0, gen_token, greedy, copyLogits, pSampler);
    // State by position -- the guide's automaton, Mirostat's mu -- is put to NONE at a prompt group's positions (in stream order, outside the graph, where
    // the coin ring's copy sits): the guide's while the model has a guide, the adaptive truncation's while the sampler has the launch on
    if (!gen_token && guide_stage.on(pSampler, mdl)) Q4_TRY(guide_clear_positions(mdl, pos, nsteps));
    if (!gen_token && mdl && mdl->adaptive_mu && adaptive_stage.on(pSampler, mdl)) Q4_TRY(adaptive_clear_positions(mdl, pos, nsteps));
    // q4_set_logprobs: a record launch between the classifier and the sampler. Of a generating step whose logits a stage rewrites the chosen token need
    // not be the raw logits' largest, so a greedy step keeps the raw logits aside and looks its token up behind the argmax, the way a sampled step does
    StepTail tail = {gen_token, copyLogits, greedy, greedy, false, mdl && mdl->logprobs_k >= 0 ? mdl : nullptr, mdl, pSampler, {}};
    int stage_bits = 0;
    for (int i = 0; i < N_STAGES && gen_token; i++)
        if (STAGES[i]->on(pSampler, mdl)) {
            Q4_TRY(STAGES[i]->prepare(pSampler, mdl, p, &tail.block[i]));
            stage_bits |= stage_bit(i);
            tail.lp_greedy = false;
        }
    tail.lp_pick = tail.lpm && gen_token && !tail.lp_greedy;

    if (g_use_graphs == 1) {
        GraphSet& gs = graph_set_of(s, p, w);
        // Unlike the reference, the greedy sampler kernel and the fp32 logits copy are part of the captured
        // graph (one launch per token instead of up to three); the variant index keeps them apart.
        const int variant = (gen_token ? 1 : 0) | (copyLogits ? 2 : 0) | (greedy ? 0 : 4) | (nsteps > 1 ? 8 : 0) | (tail.lpm ? 16 : 0) | (screened ? 32 : 0) | stage_bits;
        for (int i = 0; i < N_STAGES; i++)
            if (tail.block[i] && gs.block[i] != tail.block[i]) {     // another block: the graphs with this stage's launch hold a stale address
                drop_graphs(gs, stage_bit(i));
                gs.block[i] = tail.block[i];
            }
        CoinRing* ring = nullptr;
        if (!greedy) {     // the sampling kernel is part of the graph: its temperature, top-p, scratch and coin ring are baked in
            Q4_TRY(coin_ring_for(pSampler, p->seq_len, &ring));
            Q4_TRY(q4_sample_topp_prepare(pSampler));     // scratch + LDS opt-in: not capturable
            if (gs.sampler != pSampler || gs.temperature != pSampler->temperature || gs.topp != pSampler->topp || gs.coins != ring->dev) {
                drop_graphs(gs, 4);
                gs.sampler = pSampler; gs.temperature = pSampler->temperature; gs.topp = pSampler->topp; gs.coins = ring->dev;
            }
        }
        if (!gs.captured[graphIndex][variant]) {                                   // :362-371
            hipGraph_t graph = nullptr;
            Q4_HIP(hipStreamBeginCapture(g_stream, hipStreamCaptureModeGlobal));
            int rc = 0;
            // generated tokens, several steps per replay: step i + 1 takes the token step i writes -- its sampler launch leaves the
            // embedding row in s->x and the copy_embedding launch of step i + 1 is left out (the fused sequence only: level 0 is
            // the reference's 1:1 launch list)
            const bool feed = gen_token && nsteps > 1 && g_fusion >= 1;
            for (int i = 0; i < nsteps && !rc; i++) {
                rc = run_network(s->pos, p, s, w, seq_len_bin, feed && i > 0, screened);
                if (!rc) rc = step_tail(tail, p, s, w, true, ring ? ring->dev : nullptr, feed && i + 1 < nsteps);
            }
            hipError_t e = hipStreamEndCapture(g_stream, &graph);
            if (rc) { if (graph) hipGraphDestroy(graph); return rc; }
            Q4_HIP(e);
            Q4_HIP(hipGraphInstantiate(&gs.exec[graphIndex][variant], graph, nullptr, nullptr, 0));
            Q4_HIP(hipGraphDestroy(graph));
            gs.captured[graphIndex][variant] = true;
            g_graph_captures++;
        }
        // one coin per step, drawn whether the step samples or not (sampler.h:45, P8); the sampled steps' coins go to the ring
        for (int i = 0; i < nsteps; i++) {
            const float coin = random_f32(&pSampler->rng_state);
            if (ring) ring->host[pos + i] = coin;
        }
        if (ring) Q4_HIP(hipMemcpyAsync(ring->dev + pos, ring->host + pos, (size_t)nsteps * sizeof(float), hipMemcpyHostToDevice, g_stream));
        Q4_HIP(hipGraphLaunch(gs.exec[graphIndex][variant], g_stream));          // :372 (:384: the sampler launch is in the graph)
        return Q4_OK;
    }
    Q4_TRY(run_network(s->pos, p, s, w, g_use_graphs == 2 ? seq_len_bin : seq_len, false, screened));   // :374
    return step_tail(tail, p, s, w, false, nullptr, false);
}

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
    const Model* m = model_of(s);
    if (m) {      // the Config of a Transformer the library built sits in front of its RunState
        const Transformer* t = reinterpret_cast<const Transformer*>(reinterpret_cast<const char*>(s) - offsetof(Transformer, state));
        if (start_pos > t->config.seq_len) return Q4_ERR_ARG;
    }
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

// How many steps a token loop may queue at once from `pos`: Q4_MULTI_STEPS when graphs are on, the sampler is greedy, the
// whole group generates (or the whole group feeds prompt tokens), ends by `steps` and stays inside one sequence-length
// bin; else 1.
int q4_steps_that_fit(int pos, int num_prompt_tokens, int steps, const Config* p, const Sampler* sampler) {
    const int k = g_multi_steps;
    if (k <= 1 || g_use_graphs != 1 || pos + k > steps || pos + k > p->seq_len) return 1;
    const bool gen0 = pos >= num_prompt_tokens - 1, gen1 = pos + k - 1 >= num_prompt_tokens - 1;
    if (gen0 != gen1) return 1;
    (void)sampler;     // sampled steps take their coins from a device ring by position: they go out k per replay too
    int b0, b1;
    if (graph_bin(pos + 1, p, &b0) != graph_bin(pos + k, p, &b1)) return 1;
    // A model that screens its greedy steps: the last step a generation queues goes out alone, so that it can run the full classifier and leave
    // RunState::logits whole (group_may_screen, q4_loop.h). The Config of a Transformer leads to its record; any other Config finds none and changes nothing.
    if (pos + k == steps && gen0 && sampler && sampler->temperature == 0.0f) {
        const RunState* rs = reinterpret_cast<const RunState*>(reinterpret_cast<const char*>(p) - offsetof(Transformer, config) + offsetof(Transformer, state));
        if (step_screens(model_of(rs), true, 1, true, 0, sampler)) return 1;
    }
    return k;
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

// After a pass over a sequence: q4_handoff_status into *rc, and what every loop of this file does with a timed-out in-launch wait. The library has
// dropped to fusion level 1 and cleared its state, so the first time-out of a pass that can be repeated (redoable) puts the sampler back to rng0 and
// asks for the pass once more; any other is the error.
static bool redo_after_timeout(const RunState* s, Sampler* sampler, unsigned long long rng0, bool redoable, int* rc) {
    *rc = q4_handoff_status(s);
    if (!*rc || !redoable) return false;
    sampler->rng_state = rng0;
    return true;
}

// generate() llama2_q4.cu:436-492, the one token loop behind q4_generate and q4_generate_ids_from (q4_loop.h): same loop order -- synchronise, launch
// step `pos`, then look at the token produced by the PREVIOUS step; same throughput rule (pos-1)/elapsed. It starts at start_pos over K / V rows
// [0, start_pos) that are already in place (q4_resume_sequence's contract) and draws one coin per step whether or not the step samples, so the skipped
// steps' coins are drawn and discarded first: with the same seed a resumed sampled generation produces the full one's tokens, and a reused Sampler
// stands where the full run leaves it. q4_set_context_shift: the loop shifts at seq_len instead of stopping there, so steps may pass it; `pos` counts
// steps, and the device runs step `pos` at position pos - off, off being the positions discarded so far.
int q4_token_loop(Transformer* t, Sampler* sampler, const int* prompt_tokens, int num_prompt_tokens, int steps, int start_pos, TokenLoop* loop) {
    Model* const sm = model_of(&t->state);
    const int seq_len = t->config.seq_len, shift_keep = sm ? sm->shift_keep : 0, shift_discard = sm ? sm->shift_discard : 0;
    // the full loop stops at the first EOS it meets in the ring behind index 0, a prompt's included: a prefix that holds one is not skipped
    for (int i = 1; i < start_pos; i++)
        if (prompt_tokens[i] == 2) start_pos = 0;
    const unsigned long long rng0 = sampler->rng_state;
    for (int attempt = 0;; attempt++) {
        struct timespec t0, t1;
        clock_gettime(CLOCK_MONOTONIC, &t0);
        const int start = attempt == 0 ? start_pos : 0;      // the retry after a time-out trusts no row
        int pos = start, queued = start, group_start = start, off = 0;
        int verify_pos = -1, verify_drafts = 0;              // a verify pass queued at verify_pos whose outcome the host has not read yet
        Q4_TRY(start == 0 ? q4_reset_sequence(&t->state, prompt_tokens, num_prompt_tokens) : q4_resume_sequence(&t->state, prompt_tokens, num_prompt_tokens, start));
        if (loop->on_attempt) loop->on_attempt(loop->ctx, attempt, start);
        for (int i = 0; i < start; i++) (void)random_f32(&sampler->rng_state);
        unsigned long long group_rng = sampler->rng_state;   // sampler state in front of the group of steps queued last
        int prev = prompt_tokens[start > 0 ? start - 1 : 0];
        bool stopped = false;
        while (pos < steps) {
            if (verify_pos >= 0 && pos == verify_pos + 1) {      // the pass's advance says how many drafts it accepted: one coin per position it ran, as the steps draw them
                Q4_TRY(q4_wait_pos(&t->state, pos));
                const int m = t->state.shared_data->pos - pos;
                if (m < 0 || m > verify_drafts) return Q4_ERR_HIP;
                for (int i = 0; i <= m; i++) (void)random_f32(&sampler->rng_state);
                sm->spec_passes++;
                sm->spec_drafted += verify_drafts;
                sm->spec_accepted += m;
                queued = pos + m;
                verify_pos = -1;
            }
            // the reference synchronises and then launches step `pos` (:468-470); here the launch goes out first, queued
            // behind step pos-1, and the host then waits for step pos-1's token -- same device order, no idle gap per token.
            // Steps inside one bin go out Q4_MULTI_STEPS at a time (one graph replay); a stop at EOS leaves at most
            // Q4_MULTI_STEPS - 1 surplus steps behind, which the next q4_reset_sequence discards.
            if (pos >= queued) {
                if (shift_discard > 0 && pos - off == seq_len) {     // the wall: q4_shift_context synchronises (everything queued has finished), then the rows slide
                    Q4_TRY(q4_shift_context(t, seq_len, shift_keep, shift_discard, seq_len + 1));
                    off += shift_discard;
                }
                const int np = prompt_pass_tokens(t, sm, sampler, pos - off, num_prompt_tokens - off, steps - off, off);
                // Speculation (q4_set_speculative; spec_verify.h): at a generating position whose verify pass is admitted the host waits for the ring's
                // entry `pos` -- everything queued so far -- and asks the drafter. The entry itself is looked at below, like any other: an EOS there stops the
                // loop, and the pass queued behind it is surplus, as surplus steps are. No draft: the steps below, and the question again behind them.
                int nd = 0, draft[VERIFY_MAX_DRAFT];
                if (!np && sm && sm->spec_draft > 0 && pos >= num_prompt_tokens - 1 && verify_covers(t, sm, sampler, pos, 1, steps, off)) {
                    Q4_TRY(q4_wait_pos(&t->state, pos));
                    int room = sm->spec_draft;
                    while (room > 1 && !verify_covers(t, sm, sampler, pos, room, steps, off)) room--;
                    if (pos == 0 || t->state.shared_data->tokens[pos] != 2)      // (behind an EOS the loop stops: no pass)
                        nd = ask_drafter(sm, (const int*)t->state.shared_data->tokens, pos + 1, room, t->config.vocab_size, draft);
                }
                const int k = np ? np : nd ? 1 : q4_steps_that_fit(pos - off, num_prompt_tokens - off, steps - off, &t->config, sampler);
                group_start = pos;
                group_rng = sampler->rng_state;
                if (nd) {      // positions pos .. pos + m run, m the accepted drafts: known once the pass has published its position
                    // under the sampler (q4_set_speculative_sampled): the coins of positions pos .. pos + nd go to the ring and the stream is put back; the m + 1
                    // draws above, once m is known, leave it where the steps would
                    Sampler* const vs = sampler->temperature != 0.0f ? sampler : nullptr;
                    const float* coins = nullptr;
                    if (vs) Q4_TRY(stage_pass_coins(vs, &t->config, pos, nd, &coins));
                    Q4_TRY(run_verify_pass(&t->config, &t->state, &t->weights, sm, pos, draft, nd, vs, coins));
                    verify_pos = pos;
                    verify_drafts = nd;
                } else if (np) {      // the prompt-only positions pos .. pos + np - 1 in one pass over the weights; one coin per position, as the steps draw them
                    for (int i = 0; i < np; i++) (void)random_f32(&sampler->rng_state);
                    Q4_TRY(run_prompt_pass(&t->config, &t->state, &t->weights, sm, pos - off, np));
                    g_prompt_passes++;
                } else {
                    Q4_TRY(run_transformer_steps_screenable(pos - off, k, pos >= num_prompt_tokens - 1, &t->config, &t->state, &t->weights, 0, sampler, group_may_screen(pos - off, k, steps - off)));
                }
                queued = pos + k;
            }
            Q4_TRY(q4_wait_pos(&t->state, pos - off));                                 // :468
            if (pos > 0) {
                int next = t->state.shared_data->tokens[pos - off];                    // :473, output token of the previous iteration
                if (loop->on_token) loop->on_token(loop->ctx, pos, prev, next);
                if (next >= t->config.vocab_size) next = 0;                            // :474
                if (next == 2) { stopped = true; break; }                              // eos_token, :477
                prev = next;
            }
            pos++;
        }
        clock_gettime(CLOCK_MONOTONIC, &t1);                                           // :485, taken where the reference takes it
        if (stopped) {
            // the reference has drawn one coin per run_transformer call, steps 0..pos (sampler.h:45); a multi-step group drew
            // for its surplus steps too: put the stream back to exactly pos + 1 draws so a reused Sampler continues like the reference's
            sampler->rng_state = group_rng;
            for (int i = group_start; i <= pos; i++) (void)random_f32(&sampler->rng_state);
        }
        loop->pos = pos;
        loop->start = start;
        loop->off = off;
        loop->seconds = (t1.tv_sec - t0.tv_sec) + 1e-9 * (t1.tv_nsec - t0.tv_nsec);
        int rc;
        if (!redo_after_timeout(&t->state, sampler, rng0, attempt == 0 && off == 0, &rc)) return rc;   // (shifted rows cannot be redone)
    }
}

// ... on token ids (no tokenizer, no printing): out_tokens receives the ring by step, the evicted tokens of a run that shifts too
static void record_token(void* out_tokens, int step, int, int token) { ((int*)out_tokens)[step] = token; }
double q4_generate_ids(Transformer* t, Sampler* sampler, const int* prompt_tokens, int num_prompt_tokens, int steps,
                       int* out_tokens, int* timed_tokens_out, double* seconds_out) {
    return q4_generate_ids_from(t, sampler, prompt_tokens, num_prompt_tokens, steps, 0, out_tokens, timed_tokens_out, seconds_out);
}
double q4_generate_ids_from(Transformer* t, Sampler* sampler, const int* prompt_tokens, int num_prompt_tokens, int steps, int start_pos,
                            int* out_tokens, int* timed_tokens_out, double* seconds_out) {
    if (!t || !sampler || !prompt_tokens || num_prompt_tokens < 1) return -1.0;
    const Model* sm = model_of(&t->state);
    const int limit = sm && sm->shift_discard > 0 ? Q4_MAX_SEQ_LEN - 1 : t->config.seq_len;   // (a model that shifts generates past seq_len)
    if (steps <= 0) steps = t->config.seq_len;
    else if (steps > limit) steps = limit;                                             // :690
    if (start_pos < 0 || start_pos > num_prompt_tokens - 1 || start_pos > t->config.seq_len) {
        snprintf(g_last_error, sizeof(g_last_error), "q4_generate_ids_from: start_pos %d outside [0, %d] (%s)", start_pos, num_prompt_tokens - 1, q4_status_string(Q4_ERR_ARG));
        return -1.0;
    }
    TokenLoop loop = {out_tokens ? record_token : nullptr, nullptr, out_tokens};
    if (q4_token_loop(t, sampler, prompt_tokens, num_prompt_tokens, steps, start_pos, &loop)) return -1.0;
    if (out_tokens) {      // up to the step it started from the ring is the prompt; a run that ends at `steps` has not looked at its last token
        for (int i = 0; i <= loop.start && i <= steps; i++) out_tokens[i] = prompt_tokens[i];
        if (loop.pos == steps) out_tokens[steps] = t->state.shared_data->tokens[steps - loop.off];
    }
    const int timed_tokens = loop.pos - 1 - loop.start;                                // :488, over the steps this call ran
    if (timed_tokens_out) *timed_tokens_out = timed_tokens;
    if (seconds_out) *seconds_out = loop.seconds;
    return loop.seconds > 0 ? timed_tokens / loop.seconds : 0.0;
}

// ---------------------------------------------------------------------------------------------------
// perplexity.h:3-51 (host math)
void q4_softmax_f32(float* x, int size) {
    float max_val = x[0];
    for (int i = 1; i < size; i++)
        if (x[i] > max_val) max_val = x[i];
    float sum = 0.0f;
    for (int i = 0; i < size; i++) {
        x[i] = expf(x[i] - max_val);
        sum += x[i];
    }
    for (int i = 0; i < size; i++) x[i] /= sum;
}
float compute_perplexity(const int* tokens, float* logits, int num_tokens, int vocab_size) {
    double sum = 0.0;
    for (int i = 0; i < num_tokens; i++) {
        int word_index = tokens[i];
        q4_softmax_f32(&logits[(size_t)i * vocab_size], vocab_size);
        double prob = logits[(size_t)i * vocab_size + word_index];
        sum += log(prob);
    }
    double avg_log_prob = sum / num_tokens;
    return float(exp(-avg_log_prob));
}

// get_dataset_perplexity perplexity.h:57-97 on token ids: tokens_with_bos[0] = BOS, targets follow.
float q4_perplexity_ids(Transformer* t, Sampler* sampler, const int* tokens_with_bos, int num_tokens) {
    Config* config = &t->config;
    RunState* state = &t->state;
    if (!state->logits_array || num_tokens < 1) return -1.0f;
    if (num_tokens >= config->seq_len) num_tokens = config->seq_len - 1;           // :68-72
    const unsigned long long rng0 = sampler->rng_state;
    int rc;
    for (int attempt = 0;; attempt++) {
        if (q4_reset_sequence(state, tokens_with_bos, num_tokens + 1)) return -1.0f;   // :76-78
        // the input tokens are all known: the steps are queued back to back (the device advances its own position) and the
        // host synchronises once, where the reference calls cudaDeviceSynchronize after every step (:81)
        for (int pos = 0; pos < num_tokens; pos++)
            if (q4_run_transformer_at(pos, 0, config, state, &t->weights, 1, sampler)) return -1.0f;   // :80
        if (hipDeviceSynchronize() != hipSuccess) return -1.0f;                        // :81
        if (!redo_after_timeout(state, sampler, rng0, attempt == 0, &rc)) break;
    }
    if (rc) return -1.0f;
    float* logits_arr = (float*)malloc((size_t)num_tokens * config->vocab_size * sizeof(float));
    if (q4_get_logits_array(t, num_tokens, logits_arr)) { free(logits_arr); return -1.0f; }   // :88-89
    float pplx = compute_perplexity(tokens_with_bos + 1, logits_arr, num_tokens, config->vocab_size);   // :91
    free(logits_arr);
    return pplx;
}

// ---------------------------------------------------------------------------------------------------
// log-probability records (q4_logprobs.hip): the per-model switch, the read-out, teacher-forced scoring. Not in the reference.
int q4_set_logprobs(Transformer* t, int top_k) {
    if (!t || top_k < -1 || top_k > Q4_MAX_TOP_LOGPROBS) return Q4_ERR_ARG;
    Model* m = model_of(&t->state);
    if (!m || top_k > t->config.vocab_size) return Q4_ERR_ARG;
    if (top_k == m->logprobs_k) return Q4_OK;
    if (top_k >= 0 && !logprobs_size_ok(t->config.vocab_size, top_k)) return Q4_ERR_UNSUPPORTED_SIZE;
    const size_t S = (size_t)t->config.seq_len, K = (size_t)(top_k < 0 ? 0 : top_k);
    const size_t side = ((size_t)t->config.vocab_size * sizeof(q4_half) + 255) / 256 * 256;
    const size_t bytes = side + S * sizeof(float) * 2 + S * K * (sizeof(int) + sizeof(float));
    void* ring = nullptr;                                                          // the new ring first: a failed allocation leaves the setting as it was
    if (top_k >= 0 && hipMalloc(&ring, bytes) != hipSuccess) { (void)hipGetLastError(); return Q4_ERR_ALLOC; }
    drop_logprob_graphs_of(&t->state);
    (void)hipStreamSynchronize(g_stream);                                         // an eager launch may still be writing the old ring
    if (m->lp_ring) (void)hipFree(m->lp_ring);
    m->lp_ring = nullptr; m->lp_lse = m->lp_token = m->lp_top = nullptr; m->lp_ids = nullptr; m->lp_side = nullptr;
    m->logprobs_k = -1;
    if (top_k < 0) return Q4_OK;
    m->lp_ring = ring;
    Q4_HIP(hipMemsetAsync(m->lp_ring, 0, bytes, g_stream));
    Q4_HIP(hipStreamSynchronize(g_stream));
    char* c = (char*)m->lp_ring;
    m->lp_side = (q4_half*)c; c += side;
    m->lp_lse = (float*)c; c += S * sizeof(float);
    m->lp_token = (float*)c; c += S * sizeof(float);
    m->lp_ids = (int*)c; c += S * K * sizeof(int);
    m->lp_top = (float*)c;
    m->logprobs_k = top_k;
    return Q4_OK;
}
int q4_get_logprobs_k(const Transformer* t) {
    const Model* m = t ? model_of(&t->state) : nullptr;
    return m ? m->logprobs_k : -1;
}
int q4_get_logprobs(const Transformer* t, int first_pos, int n, float* token_logprob, int* top_ids, float* top_logprobs) {
    const Model* m = t ? model_of(&t->state) : nullptr;
    if (!m || m->logprobs_k < 0 || first_pos < 0 || n < 0 || (long long)first_pos + n > t->config.seq_len) return Q4_ERR_ARG;
    Q4_HIP(hipStreamSynchronize(g_stream));
    const size_t K = (size_t)m->logprobs_k, f = (size_t)first_pos;
    if (n == 0) return Q4_OK;
    if (token_logprob) Q4_HIP(hipMemcpy(token_logprob, m->lp_token + f, (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
    if (top_ids && K) Q4_HIP(hipMemcpy(top_ids, m->lp_ids + f * K, (size_t)n * K * sizeof(int), hipMemcpyDeviceToHost));
    if (top_logprobs && K) Q4_HIP(hipMemcpy(top_logprobs, m->lp_top + f * K, (size_t)n * K * sizeof(float), hipMemcpyDeviceToHost));
    return Q4_OK;
}
int q4_score_ids(Transformer* t, Sampler* sampler, const int* tokens_with_bos, int num_tokens, float* logprobs_out) {
    if (!t || !sampler || !tokens_with_bos || !logprobs_out || num_tokens < 1) return Q4_ERR_ARG;
    Config* config = &t->config;
    RunState* state = &t->state;
    const Model* m = model_of(state);
    if (!m || num_tokens > config->seq_len - 1) return Q4_ERR_ARG;
    const int before = m->logprobs_k;
    if (before < 0) Q4_TRY(q4_set_logprobs(t, 0));
    const unsigned long long rng0 = sampler->rng_state;
    int rc;
    for (int attempt = 0;; attempt++) {
        rc = q4_reset_sequence(state, tokens_with_bos, num_tokens + 1);
        // every input token is known: the steps go out like generate()'s prompt steps (a target is the NEXT ring entry), up to Q4_MULTI_STEPS per replay
        for (int pos = 0; pos < num_tokens && !rc;) {
            const int k = q4_steps_that_fit(pos, num_tokens + 1, num_tokens, config, sampler);
            rc = q4_run_transformer_steps(pos, k, 0, config, state, &t->weights, 0, sampler);
            pos += k;
        }
        if (!rc && hipStreamSynchronize(g_stream) != hipSuccess) rc = Q4_ERR_HIP;
        if (rc || !redo_after_timeout(state, sampler, rng0, attempt == 0, &rc)) break;
    }
    if (!rc) rc = q4_get_logprobs(t, 0, num_tokens, logprobs_out, nullptr, nullptr);
    if (before < 0) { const int rc2 = q4_set_logprobs(t, -1); if (!rc) rc = rc2; }
    return rc;
}

}  // extern "C"
