// q4_loops.hip -- the loops over the step: the one generate loop (q4_token_loop, q4_loop.h: q4_generate_ids and q4_host.cpp's q4_generate) over steps, prompt
// passes and verify passes; perplexity and scoring on token ids. Mirrors llama2_q4.cu:436-492 (generate), perplexity.h:3-51 and :57-97.
#include <math.h>
#include <stdlib.h>
#include <time.h>
#include "q4_model.h"
#include "q4_loop.h"
#include "prompt_pass.h"
#include "spec_verify.h"

using namespace q4;

extern "C" {

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
        bool verify_forced = false;                          // ... whose drafts are the guide's forced run (q4_spec_stats_forced)
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
                count_verify_pass(sm, verify_drafts, m, verify_forced);
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
                // (dmin: the fewest drafts a verify pass of this shape takes -- prompt_pass_min rows, 1 draft but for Llama-2-13B's shape; a shorter draft runs steps)
                const int dmin = prompt_pass_min(&t->config) - 1;
                if (!np && sm && sm->spec_draft >= dmin && pos >= num_prompt_tokens - 1 && verify_covers(t, sm, sampler, pos, dmin, steps, off)) {
                    Q4_TRY(q4_wait_pos(&t->state, pos));
                    int room = sm->spec_draft;
                    while (room > dmin && !verify_covers(t, sm, sampler, pos, room, steps, off)) room--;
                    verify_forced = false;
                    if (pos == 0 || t->state.shared_data->tokens[pos] != 2) {    // (behind an EOS the loop stops: no pass)
                        // q4_set_pass_stages with a guide: where the automaton's state behind ring[pos] leaves one live token, the next tokens are known
                        // before the model runs -- the forced run first, the model's drafter only where it is empty
                        if (sm->pass_stages && sm->guide) Q4_TRY(guide_forced_draft(sm, (const int*)t->state.shared_data->tokens, pos, room, draft, &nd));
                        if (nd < dmin) nd = 0;
                        verify_forced = nd > 0;
                        if (!nd) nd = ask_drafter(sm, (const int*)t->state.shared_data->tokens, pos + 1, room, t->config.vocab_size, draft);
                        if (nd < dmin) nd = 0;
                    }
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
                    Q4_TRY(run_verify_pass(&t->config, &t->state, &t->weights, sm, pos, draft, nd, vs, coins, sampler));
                    verify_pos = pos;
                    verify_drafts = nd;
                } else if (np) {      // the prompt-only positions pos .. pos + np - 1 in one pass over the weights; one coin per position, as the steps draw them
                    for (int i = 0; i < np; i++) (void)random_f32(&sampler->rng_state);
                    Q4_TRY(run_prompt_pass(&t->config, &t->state, &t->weights, sm, pos - off, np, sampler));
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

// Teacher-forced scoring through the log-probability records (q4_logprobs.hip). Not in the reference. (q4_perplexity_ids above keeps its steps: the fp32
// logits_array path is the reference's, one copy per token.)
int q4_score_ids(Transformer* t, Sampler* sampler, const int* tokens_with_bos, int num_tokens, float* logprobs_out) {
    if (!t || !sampler || !tokens_with_bos || !logprobs_out || num_tokens < 1) return Q4_ERR_ARG;
    Config* config = &t->config;
    RunState* state = &t->state;
    Model* m = model_of(state);
    if (!m || num_tokens > config->seq_len - 1) return Q4_ERR_ARG;
    const int before = m->logprobs_k;
    if (before < 0) Q4_TRY(q4_set_logprobs(t, 0));
    const unsigned long long rng0 = sampler->rng_state;
    int rc;
    for (int attempt = 0;; attempt++) {
        rc = q4_reset_sequence(state, tokens_with_bos, num_tokens + 1);
        // every input token is known: the steps go out like generate()'s prompt steps (a target is the NEXT ring entry), up to Q4_MULTI_STEPS per replay.
        // q4_set_pass_logprobs: where a prompt pass is admitted it takes up to PROMPT_PASS_MAX positions on one read of the weights and leaves their records
        // and the last one's logits (prompt_pass.h); every position of this call is prompt-only, so a pass may include the last. One coin per position, as the
        // steps draw them. The redo after a time-out runs at fusion level 1: steps.
        for (int pos = 0; pos < num_tokens && !rc;) {
            const int np = m->pass_logprobs ? prompt_pass_tokens(t, m, sampler, pos, num_tokens + 1, num_tokens, 0) : 0;
            if (np >= 2) {
                for (int i = 0; i < np; i++) (void)random_f32(&sampler->rng_state);
                rc = run_prompt_pass(config, state, &t->weights, m, pos, np, sampler);
                g_prompt_passes++;
                pos += np;
                continue;
            }
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
