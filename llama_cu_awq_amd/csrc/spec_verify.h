// spec_verify.h -- a verify pass of speculative greedy decoding (spec_verify.hip): the token at the current position p plus D drafted
// tokens (1 <= D <= VERIFY_MAX_DRAFT) run as the n = D + 1 positions p .. p + D of ONE pass over the weights -- the prompt pass's layer launches
// (prompt_pass.h), then the final norm and the classifier for all n residual rows on one read of wcls, then one launch that takes each row's greedy
// token, counts the m leading drafts the rows confirm and leaves what m + 1 greedy steps would have left. Every row's logits are, bit for bit, the logits
// the per-token step computes at that position, so the tokens a pass emits are the tokens plain greedy decoding emits.
//
// What a pass leaves: ring[p + 1 .. p + m + 1] (the confirmed drafts and the token behind them), both position words = p + m + 1, RunState::logits = row
// m's logits, RunState::x = row m's residual stream, and the K / V rows p .. p + D of every layer. Rows p + m + 1 .. p + D were computed from drafts that
// were NOT confirmed: they lie at or above the device position, which is where q4_common_prefix, q4_resume_sequence and snapshots stop trusting rows, and
// the next step or pass at those positions writes them again. Drafts travel by value in a kernel argument: an unconfirmed token never enters the ring or
// pinned memory. Every dependency is a launch boundary: the pass waits on nothing in-launch and touches neither the model's hand-off words nor its
// granules (the attention launch writes the prompt pass's own sink).
// A model with the FP8 cache (q4_set_pass_kv8; prompt_pass_kv8.h): the layer loop's append launch writes the e4m3 bytes and both row exponents of rows
// p .. p + D, those of rejected drafts included -- they too lie at or above the device position and are rewritten (bytes and exponents) by the step or the
// pass that runs there next, as on the fp16 cache.
//
// Under the temperature / top-p sampler (q4_set_speculative_sampled): a sampled step is a function of its logits and one coin, and the coin is a function
// of (seed, position) that reaches the device through the coin ring by position. So between the classifier and the accept launch every row is sampled in
// place with its own position's coin, exactly as the step at that position would (the row form of the two sampler launches, q4_sampling.hip), and the
// accept launch takes those tokens instead of the rows' argmax: the leading drafts that equal the sampled tokens are accepted, RunState::logits receives
// row m's fp16 probabilities -- what the sampled step leaves there --, and the run is the run without passes for that seed, byte for byte.
//
// With log-probability records on (admitted only with q4_set_pass_logprobs on): the row form of the record launch (q4_logprobs.hip) goes between the
// classifier and the accept launch -- greedy: a row's token_logprob is entry 0 of its top order; under the sampler: the raw rows go to the pass's side rows
// in front of the sampler's row form and a row form of the look-up fills token_logprob behind it from the rows' tokens. Records p .. p + m are what m + 1
// steps write. Records p + m + 1 .. p + D describe rejected drafts: they lie at or above the device position and are rewritten by whatever runs there
// next -- the same contract as the K / V rows of rejected drafts.
//
// Under the logit stages (admitted only with q4_set_pass_stages on): between the record launch's place and the sampler's row form / the accept launch every
// stage that is on rewrites the rows in place through its row form (LogitStage::launch_rows), block r at position p + r, exactly as the step at that position
// would. A stage reads tokens by position, and rows behind the first stand on drafts, which never enter the ring: one launch in front of the stage rows fills
// the model's draft view (PassScratch::view, seq_len ints by absolute position) -- view[lo .. p] from the ring, view[p + 1 .. p + D] from the kernel
// argument, lo = max(0, p + 1 - Q4_MAX_DRY_WINDOW): the lowest entry any stage's step form reads at a position p .. p + D (DRY's window of at most 4096
// entries, whose walk-back stays inside it; the penalties' of at most 1024; the guide's tokens[p + r]). The guide's state ring receives p .. p + D; the
// states of rejected drafts lie at or above the device position and are rewritten by whatever runs there next -- the K / V rows' contract.
#pragma once
#include "prompt_pass.h"

namespace q4 {

constexpr int VERIFY_MAX_DRAFT = PROMPT_PASS_MAX - 1;
static_assert(VERIFY_MAX_DRAFT == Q4_SPEC_MAX_DRAFT, "the public bound on a pass's drafts is the kernel argument's capacity");

struct VerifyDrafts { int n; int tok[VERIFY_MAX_DRAFT]; };
// *out from draft[0 .. n_draft). Q4_ERR_ARG: draft null, n_draft outside [1, VERIFY_MAX_DRAFT], an id outside [0, vocab) (vocab < 0: ids are not checked)
int verify_drafts(const int* draft, int n_draft, int vocab, VerifyDrafts* out);

// Geometry the classifier launch of a pass takes: dim 4096 or 5120 (eight or ten 1 KiB pieces per vocabulary row) and a vocabulary that is a multiple of 8 -- both forms
// classifier_with_final_norm can take for such a model (strips, or rmsnorm_kernel + gemv_f16_kernel) round the same sums in the same order.
bool verify_cls_covers(int dim, int vocab);
// logits [n][vocab] = wcls . rmsnorm(x[t], rms_w) for rows t < n <= PROMPT_PASS_MAX, x [n][dim]; on the launch stream
int launch_verify_cls(q4_half* logits, const q4_half* x, const q4_half* rms_w, const q4_half* wcls, int dim, int vocab, int n);
// The accept launch. logits: rows of `size` halves `ld` apart (ld a multiple of 8: rows stay 16-byte aligned), row t the logits at position *pPosGpu + t;
// x: rows of dim halves. report (device, 9 ints, may be null): the rows' tokens and, in [8], m. win null: a row's token is its argmax.
// Else the rows' tokens are given (win, device, d.n + 1 ints) instead of each row's argmax: the pass under the sampler. The rows then hold what the row form
// of the sampler left in place -- fp16 probabilities, which is what a sampled step leaves in RunState::logits -- and everything behind the tokens is the same.
int launch_verify_accept(const q4_half* logits, int ld, int size, const VerifyDrafts& d, const int* win, const q4_half* x, int dim, q4_half* logits_out,
                         q4_half* x_out, int* ring, volatile int* pPos, int* pPosGpu, int* report);
// The row form of the temperature / top-p sampler (q4_sampling.hip): rows t < n_rows of logits, `ld` halves apart, each normalised IN PLACE and searched as
// the sampled step does for that row alone -- softmax_spread_kernel's and topp_sample_kernel<true>'s arithmetic, one grid slice per row -- with the coin
// coins[*pPosGpu + t] (coins[t] where pPosGpu is null); win[t] = the row's token and nothing else is written. Only the on-chip form: a vocabulary of at most
// 32 x 1024 entries, a multiple of 8, and a finite temperature above 0 (sample_rows_covers). sample_rows_prepare allocates the per-row scratch beside the
// Sampler on first use (outside the launch path); destroy_sampler releases it.
bool sample_rows_covers(const Sampler* sampler);
int sample_rows_prepare(Sampler* sampler);
int launch_sample_rows(Sampler* sampler, q4_half* logits, int ld, int n_rows, const float* coins, int* pPosGpu, int* win);
void sample_rows_release(const Sampler* sampler);
// The whole pass at the device position, which the caller knows to be pos0 (q4_passes.hip's verify_covers has admitted it there). On the launch stream;
// nothing is waited for. sampler null: greedy. Else the pass under that sampler: behind the classifier the rows are sampled (coins: the device coin ring by
// position, entries pos0 .. pos0 + n_draft drawn by the caller) and the accept launch takes those tokens.
// stages: the Sampler whose logit stages (and the model's guide) rewrite the rows in front of that -- also a greedy one's; null: the model's guide alone (the greedy primitive). The caller's
// admission has found every stage that is on to have a row form.
int run_verify_pass(const Config* p, RunState* s, const TransformerWeights* w, Model* m, int pos0, const int* draft, int n_draft, Sampler* sampler = nullptr,
                    const float* coins = nullptr, const Sampler* stages = nullptr);
// q4_passes.hip. The admission of a pass at `pos` (sampler null: the primitive's greedy form); the drafter's answer for ring[0 .. n_tokens); q4_spec_stats' counters
bool verify_covers(const Transformer* t, const Model* m, const Sampler* sampler, int pos, int n_draft, int steps, int off);
int ask_drafter(const Model* m, const int* ring, int n_tokens, int max_draft, int vocab, int* draft);
void count_verify_pass(Model* m, int n_draft, int accepted, bool forced = false);
// q4_step.hip (the coin ring lives there). The coins of positions pos .. pos + n_draft into the sampler's device ring, the sampler's stream put back
int stage_pass_coins(Sampler* sampler, const Config* p, int pos, int n_draft, const float** coins_dev);

}  // namespace q4
