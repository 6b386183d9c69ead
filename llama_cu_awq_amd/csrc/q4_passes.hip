// q4_passes.hip -- when a prompt pass or a verify pass (prompt_pass.h, spec_verify.h) may stand in for per-token steps: the admission,
// the speculative settings and the built-in drafter, the verify primitive's host side. Not in the reference (one step per token, llama2_q4.cu:436-492).
#include <stdlib.h>
#include <string.h>
#include "q4_model.h"
#include "prompt_pass.h"
#include "spec_verify.h"
#include "option_text.h"

namespace q4 {

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
    const Model* m = model_of(s);
    const bool kv8 = m && m->kv_format == Q4_KV_FP8;
    for (int i = 0; i < n; i++) {
        const int arg_i = step_bin_arg(p, pos + i);
        if (kv8) {
            // The FP8 cache: the form launch_attention_kv8 takes at this position (its own predicate), in this plan's terms -- the one-pass form up to bin
            // argument 256 (the row form keeps 256 scores) as 5, the split-context form by its chunk as 2 (128 positions) or 3 (256); a one-pass step above
            // 256 (no graphs: arguments 257 .. 511; records that do not fit the scratch) has no row form
            if (arg_i != arg) {
                const Kv8Form f = attention_kv8_form(p->n_heads, head_size, arg_i, s->att != nullptr, att_buffer_bytes(p));
                form = f.split ? (f.chunk == 128 ? 2 : 3) : arg_i <= PASS_CONTEXT_MIN ? 5 : -1;
            }
        } else if (arg_i != arg) form = attention_oproj_form(p->dim, kv_dim, head_size, p->n_heads, arg_i, s->att != nullptr, att_buffer_bytes(p), g_att_split_min, g_att_chunk);
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
// prompt_pass_covers admits (fp16 cache, or the FP8 cache with q4_set_pass_kv8 on; unmasked stream); every position prompt-only, inside `steps`, below the bound of q4_set_pass_context and inside
// the bin of `pos`; no log-probability records (they describe prompt steps' logits) or q4_set_pass_logprobs on (pass_records_ok: the pass then runs the
// classifier and writes the records); neither the guide nor the adaptive truncation on unless the model's q4_set_pass_stages switch is (their state by
// position is put to NONE per prompt step); no context-shift offset. (copyLogits: a token loop never asks for it.) q4_score_ids asks too, with that
// switch on: there every position is prompt-only (num_prompt_tokens = steps + 1).
// Records and passes: records off, nothing to ask. On, a pass is taken only with the model's q4_set_pass_logprobs switch on and a shape that the pass's
// classifier (a prompt pass then runs the verify pass's) and the row form of the record launch take.
static bool pass_records_ok(const Config* p, const Model* m) {
    return m->logprobs_k < 0 || (m->pass_logprobs && verify_cls_covers(p->dim, p->vocab_size) && logprobs_size_ok(p->vocab_size, m->logprobs_k));
}
static int g_prompt_ingest = PROMPT_PASS_MAX;
int g_prompt_passes = 0;
int prompt_pass_tokens(const Transformer* t, const Model* m, const Sampler* sampler, int pos, int num_prompt_tokens, int steps, int off) {
    if (g_prompt_ingest < 2 || g_fusion < 3 || off != 0 || !m || !pass_records_ok(&t->config, m)) return 0;
    const Config* p = &t->config;
    int n = num_prompt_tokens - 1 - pos;
    if (n > g_prompt_ingest) n = g_prompt_ingest;
    if (n > steps - pos) n = steps - pos;
    if (n > pass_bin_end(pos) - pos) n = pass_bin_end(pos) - pos;
    if (n > pass_bound(p) - pos) n = pass_bound(p) - pos;
    // (state by position: the steps put it to NONE per prompt group; with q4_set_pass_stages on run_prompt_pass does the same)
    if (n < prompt_pass_min(p) || (!m->pass_stages && (guide_stage.on(sampler, m) || adaptive_stage.on(sampler, m))) || !prompt_pass_covers(p, m)) return 0;
    PassAttention plan;
    return pass_attention_plan(p, &t->state, pos, n, &plan) ? n : 0;
}

// A verify pass (spec_verify.h) at position `pos` with n_draft drafts, positions pos .. pos + n_draft: what a prompt pass requires -- the
// fusion level in force >= 3 with an attention form the pass reproduces at every position (pass_attention_plan), prompt_pass_covers' geometry (fp16 cache,
// unmasked stream), no log-probability records or q4_set_pass_logprobs on (pass_records_ok), no guide unless q4_set_pass_stages is on, no context-shift offset, every position inside the bin of `pos`, below the bound of
// q4_set_pass_context and inside seq_len -- plus a classifier shape the pass's launch
// takes. A token loop adds (sampler non-null): temperature 0 -- or, with the model's spec_sampled switch on, a sampler the row form of the sampling
// launches takes (sample_rows_covers) --, no logit stage on (q4_set_pass_stages: none without a row form, and none together with records), every position inside `steps`. With all of that off a greedy generating
// step leaves, by position: its K / V rows, ring[pos + 1], the two position words; and, not by position: RunState::logits, RunState::x (un-normalised
// behind the strips classifier; what the pass writes), the scratch vectors xb / hb / q / att (rewritten by every step before it reads them), the hand-off
// epoch (never rewound; a pass does not advance it, as a prompt pass does not), the screen's tallies (q4_screen_candidates counts screened steps: a pass
// screens nothing). Guide states, Mirostat's mu, the coin ring and logits_array are written only by what the admission excludes; the record rings by the
// pass itself where q4_set_pass_logprobs admits it with records on (spec_verify.h: records p .. p + D, those of rejected drafts at or above the position).
bool verify_covers(const Transformer* t, const Model* m, const Sampler* sampler, int pos, int n_draft, int steps, int off) {
    if (g_fusion < 3 || off != 0 || !m || !pass_records_ok(&t->config, m) || n_draft < 1 || n_draft > VERIFY_MAX_DRAFT || pos < 0) return false;
    const Config* p = &t->config;
    if (pos + n_draft >= pass_bin_end(pos) || pos + n_draft >= pass_bound(p) || pos + n_draft >= steps || n_draft + 1 < prompt_pass_min(p)) return false;
    if (sampler && sampler->temperature != 0.0f) {
        // q4_set_speculative_sampled: the pass under the sampler -- the row form of its two launches (the on-chip vocabulary, a finite temperature above 0;
        // a negative one keeps the one-block softmax of the step) and a vocabulary that is the model's
        if (!m->spec_sampled || sampler->vocab_size != p->vocab_size || !sample_rows_covers(sampler)) return false;
    }
    // Logit stages (the guide is on with or without a sampler): only with q4_set_pass_stages on, every stage that is on with a row form (not the adaptive
    // truncation) and no log-probability records (a stage step keeps the raw logits aside and looks its token up behind the argmax: no row form of that)
    if (any_stage_on(sampler, m) && (!m->pass_stages || !stages_take_rows(sampler, m) || m->logprobs_k >= 0)) return false;
    if (!prompt_pass_covers(p, m) || !verify_cls_covers(p->dim, p->vocab_size)) return false;
    PassAttention plan;
    return pass_attention_plan(p, &t->state, pos, n_draft + 1, &plan);
}
// The drafter's answer for ring[0 .. n_tokens), at most max_draft ids, cut in front of the first id outside the vocabulary
int ask_drafter(const Model* m, const int* ring, int n_tokens, int max_draft, int vocab, int* draft) {
    int n = m->drafter ? m->drafter(m->drafter_ctx, ring, n_tokens, max_draft, draft) : q4_spec_draft(ring, n_tokens, max_draft, m->spec_ngram_max, m->spec_ngram_min, draft);
    if (n > max_draft) n = max_draft;
    for (int i = 0; i < n; i++)
        if (draft[i] < 0 || draft[i] >= vocab) { n = i; break; }
    return n < 0 ? 0 : n;
}
void count_verify_pass(Model* m, int n_draft, int accepted, bool forced) {
    m->spec_passes++; m->spec_drafted += n_draft; m->spec_accepted += accepted;
    if (forced) { m->forced_drafted += n_draft; m->forced_accepted += accepted; }
}

// The one host side of q4_verify_tokens and q4_verify_tokens_sampled (sampler null: the greedy form, which draws no coin). Argument errors in front of the
// synchronise, Q4_NOT_ADMITTED from rows_suspect or the admission, Q4_ERR_HIP for an advance outside [0, n_draft].
static int verify_tokens(Transformer* t, Sampler* sampler, const int* draft, int n_draft, int* out_tokens, int* n_accepted) {
    Model* m = t ? model_of(&t->state) : nullptr;
    if (!m || !out_tokens || !n_accepted) return Q4_ERR_ARG;
    VerifyDrafts d;
    Q4_TRY(verify_drafts(draft, n_draft, t->config.vocab_size, &d));      // (the arguments' check; the pass fills its own)
    Q4_HIP(hipStreamSynchronize(g_stream));
    const int pos = t->state.shared_data->pos;
    if (m->rows_suspect || !(sampler ? q4_verify_covers_sampled(t, sampler, pos, n_draft) : q4_verify_covers(t, pos, n_draft))) return Q4_NOT_ADMITTED;
    const float* coins = nullptr;
    if (sampler) Q4_TRY(stage_pass_coins(sampler, &t->config, pos, n_draft, &coins));
    Q4_TRY(run_verify_pass(&t->config, &t->state, &t->weights, m, pos, draft, n_draft, sampler, coins, sampler));
    Q4_HIP(hipStreamSynchronize(g_stream));
    const int acc = t->state.shared_data->pos - (pos + 1);
    if (acc < 0 || acc > n_draft) return Q4_ERR_HIP;
    for (int i = 0; sampler && i <= acc; i++) (void)random_f32(&sampler->rng_state);      // one coin per position that ran
    count_verify_pass(m, n_draft, acc);
    for (int i = 0; i <= acc; i++) out_tokens[i] = t->state.shared_data->tokens[pos + 1 + i];
    *n_accepted = acc;
    return Q4_OK;
}

}  // namespace q4

using namespace q4;

extern "C" {

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
int q4_verify_tokens(Transformer* t, const int* draft, int n_draft, int* out_tokens, int* n_accepted) { return verify_tokens(t, nullptr, draft, n_draft, out_tokens, n_accepted); }

// ---- verify passes under the temperature / top-p sampler (spec_verify.h): the switch, the probe, the primitive ----
int q4_set_speculative_sampled(Transformer* t, int on) {
    Model* m = t ? model_of(&t->state) : nullptr;
    if (!m) return Q4_ERR_ARG;
    m->spec_sampled = on != 0;
    return Q4_OK;
}
// Passes while the log-probability records are on (q4_set_logprobs): per model, off by default. No captured graph contains a pass: nothing to drop.
int q4_set_pass_logprobs(Transformer* t, int on) {
    Model* m = t ? model_of(&t->state) : nullptr;
    if (!m) return Q4_ERR_ARG;
    m->pass_logprobs = on != 0;
    return Q4_OK;
}
int q4_get_pass_logprobs(const Transformer* t) {
    const Model* m = t ? model_of(&t->state) : nullptr;
    return m && m->pass_logprobs ? 1 : 0;
}
// Passes for the grouped-query 4096-wide shape (prompt_pass_covers): per model, off by default. No captured graph contains a pass: nothing to drop.
int q4_set_pass_gqa(Transformer* t, int on) {
    Model* m = t ? model_of(&t->state) : nullptr;
    if (!m) return Q4_ERR_ARG;
    m->pass_gqa = on != 0;
    return Q4_OK;
}
int q4_get_pass_gqa(const Transformer* t) {
    const Model* m = t ? model_of(&t->state) : nullptr;
    return m && m->pass_gqa ? 1 : 0;
}
int q4_parse_pass_gqa(const char* text, int* on) {     // the CLI's Q4_PASS_GQA: "0" or "1", nothing else
    if (!text || !on || (text[0] != '0' && text[0] != '1') || text[1]) return Q4_ERR_ARG;
    *on = text[0] - '0';
    return Q4_OK;
}
// Passes for a model with the FP8 cache (prompt_pass_covers; prompt_pass_kv8.h): per model, off by default. No captured graph contains a pass: nothing to drop.
int q4_set_pass_kv8(Transformer* t, int on) {
    Model* m = t ? model_of(&t->state) : nullptr;
    if (!m) return Q4_ERR_ARG;
    m->pass_kv8 = on != 0;
    return Q4_OK;
}
int q4_get_pass_kv8(const Transformer* t) {
    const Model* m = t ? model_of(&t->state) : nullptr;
    return m && m->pass_kv8 ? 1 : 0;
}
int q4_parse_pass_kv8(const char* text, int* on) {     // the CLI's Q4_PASS_KV8: "0" or "1", nothing else
    if (!text || !on || (text[0] != '0' && text[0] != '1') || text[1]) return Q4_ERR_ARG;
    *on = text[0] - '0';
    return Q4_OK;
}
// Passes for Llama-2-13B's shape (prompt_pass_covers: dim 5120, hidden 13824): per model, off by default. No captured graph contains a pass: nothing to drop.
int q4_set_pass_13b(Transformer* t, int on) {
    Model* m = t ? model_of(&t->state) : nullptr;
    if (!m) return Q4_ERR_ARG;
    m->pass_13b = on != 0;
    return Q4_OK;
}
int q4_get_pass_13b(const Transformer* t) {
    const Model* m = t ? model_of(&t->state) : nullptr;
    return m && m->pass_13b ? 1 : 0;
}
int q4_parse_pass_13b(const char* text, int* on) {     // the CLI's Q4_PASS_13B: "0" or "1", nothing else
    if (!text || !on || (text[0] != '0' && text[0] != '1') || text[1]) return Q4_ERR_ARG;
    *on = text[0] - '0';
    return Q4_OK;
}
// Passes while a logit stage is on (verify passes: the guide, DRY, the sampling controls through their row forms; prompt passes: the guide, the adaptive
// truncation) and the guide's forced drafts in the token loop: per model, off by default. No captured graph contains a pass: nothing to drop.
int q4_set_pass_stages(Transformer* t, int on) {
    Model* m = t ? model_of(&t->state) : nullptr;
    if (!m) return Q4_ERR_ARG;
    m->pass_stages = on != 0;
    return Q4_OK;
}
int q4_get_pass_stages(const Transformer* t) {
    const Model* m = t ? model_of(&t->state) : nullptr;
    return m && m->pass_stages ? 1 : 0;
}
int q4_parse_pass_stages(const char* text, int* on) {     // the CLI's Q4_PASS_STAGES: "0" or "1", nothing else
    if (!text || !on || (text[0] != '0' && text[0] != '1') || text[1]) return Q4_ERR_ARG;
    *on = text[0] - '0';
    return Q4_OK;
}
int q4_spec_stats_forced(const Transformer* t, long long* drafted, long long* accepted) {
    const Model* m = t ? model_of(&t->state) : nullptr;
    if (!m) return Q4_ERR_ARG;
    if (drafted) *drafted = m->forced_drafted;
    if (accepted) *accepted = m->forced_accepted;
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
int q4_verify_tokens_sampled(Transformer* t, Sampler* sampler, const int* draft, int n_draft, int* out_tokens, int* n_accepted) { return sampler ? verify_tokens(t, sampler, draft, n_draft, out_tokens, n_accepted) : Q4_ERR_ARG; }

}  // extern "C"
