// q4_loop.h -- what q4_step.hip and q4_loops.hip keep for q4_host.cpp's drivers beside the C ABI: the step a token loop queues and the generate loop itself. Not
// exported (exports.map lists neither); plain C++ over llama2_q4.h's types, no HIP.
#pragma once
#include "llama2_q4.h"

#define Q4_PRIVATE extern "C" __attribute__((visibility("hidden")))

// q4_run_transformer_steps for a token loop; may_screen says that nobody reads the group's logits (the greedy screen, cls_screen.h)
Q4_PRIVATE int run_transformer_steps_screenable(int pos, int nsteps, int gen_token, const Config* p, RunState* s, const TransformerWeights* w, int copyLogits,
                                                Sampler* pSampler, int may_screen);
// what a token loop passes as may_screen for the group of k steps it queues at pos: every step but the generation's last, whose logits stay whole
static inline int group_may_screen(int pos, int k, int steps) { return pos + k < steps ? 1 : 0; }

// generate(), llama2_q4.cu:436-492, once for q4_generate and q4_generate_ids_from: the whole generation from start_pos (0: from a reset) to `steps` or EOS,
// redone once from 0 after a timed-out hand-off. The callers differ in what they do with a token, so they see each one the loop looks at.
struct TokenLoop {
    // in, each may be null. on_token: ring entry `step` as the device wrote it (not clamped to the vocabulary), behind `prev`; the loop stops behind an EOS.
    // on_attempt: an attempt's sequence has begun at `start`; attempt 1 follows a time-out, and what attempt 0 reported is void.
    void (*on_token)(void* ctx, int step, int prev, int token);
    void (*on_attempt)(void* ctx, int attempt, int start);
    void* ctx;
    // out, of the last attempt: where it stopped and started (timed_tokens = pos - 1 - start), the positions context shifts discarded, its seconds
    int pos, start, off;
    double seconds;
};
// the status of the call that failed; a second time-out, and one behind a context shift (those rows cannot be redone), is q4_handoff_status's
Q4_PRIVATE int q4_token_loop(Transformer* t, Sampler* sampler, const int* prompt_tokens, int num_prompt_tokens, int steps, int start_pos, TokenLoop* loop);
