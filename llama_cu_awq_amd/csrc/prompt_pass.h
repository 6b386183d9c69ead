// prompt_pass.h -- a prompt pass: up to PROMPT_PASS_MAX consecutive prompt-only positions run layer by layer with ONE read of every weight
// (prompt_pass.hip). What q4_loops.hip's token loop, q4_passes.hip's admission and q4_model.hip see of it.
#pragma once
#include "q4_model.h"

namespace q4 {

constexpr int PROMPT_PASS_MAX = 8;      // tokens per weight read (T)
constexpr int PASS_CONTEXT_MIN = 256;   // q4_set_pass_context: the default bound, the end of the V-slice bins

// The geometry part of the admission (q4_passes.hip decides the rest): Llama-2-7B's shape -- dim 4096, multi-head, 128-wide heads, a hidden size the
// three-phase FFN launch admits (its down projection is the two-part K split in three k-slots), a rotation table, an fp16 cache, an unmasked stream.
// With the model's q4_set_pass_gqa switch on also the grouped-query shape of Mistral-7B / Llama-3-8B: dim 4096, 128-wide heads, n_heads = 4 * n_kv_heads,
// a hidden size whose down projection the step runs as the two-part K split with three whole k-slots and a shared half slot per part (14336) -- while
// the profiling knobs g_ksplit / g_half_tail leave the step that form. A multi-head model is judged as with the switch off.
// With the model's q4_set_pass_kv8 switch on also either shape with the FP8 cache (prompt_pass_kv8.h): 128-wide heads, both exponent arrays in place.
// With the model's q4_set_pass_13b switch on also Llama-2-13B's shape: dim 5120 as forty 128-wide heads, multi-head, hidden 13824, an fp16 cache -- K =
// 5120 as two whole k-slots and the step's shared half slot in q/k/v, o-proj and gate/up, the down projection in the K split's shared-half-slot form --
// while the step runs the product's GEMV forms with the half slot and the K split in force (g_gemv_form, g_half_tail, g_ksplit, g_ablate). Grouped-query
// models of this width, the FP8 cache (also with q4_set_pass_kv8) and other hidden sizes keep their steps.
bool prompt_pass_covers(const Config* p, const Model* m);
// The fewest positions a pass of this shape takes (prompt passes; verify passes: drafts + 1): the smallest n at which ONE pass measured faster than n
// steps at positions 30, 300 and 2000 alike (profiles/pass_13b_bench.json). 2 at width 4096; 4 at
// Llama-2-13B's shape, where a pass of two costs 4.26 ms against 3.63 for two steps and a pass of three 5.36 against 5.27 at position 30. The kernels
// take any 2 <= n <= PROMPT_PASS_MAX (prompt_pass_layers); the admission (q4_passes.hip) and the token loop's drafts (q4_loops.hip) keep to this.
int prompt_pass_min(const Config* p);
// Which attention launch the layers of a pass over positions pos .. pos + n - 1 take (q4_passes.hip, the admission's one place): for every position the
// form of the step's attention -> o-proj launch (attention_oproj_form of the bin argument the step would hand to run_network there) is either a V-slice
// form (5 / 6: form = 5, prompt_attention_kernel) or ONE split-context form for all of them (form = 4 / 2 / 3, chunk = 64 / 128 / 256 positions:
// prompt_split_attention_kernel + prompt_merge_kernel). nsp: chunks per head the pass launches and lays its records out by; nsp_of_bin: the chunk count
// the step's launch merges in that bin, or 0 where the step is handed its own size (no graphs): ceil((position + 1) / chunk). False: no pass.
// A model with the FP8 cache: the form launch_attention_kv8 takes at every position (attention_kv8_form) -- the one-pass form with a bin argument of at most
// 256 (form = 5: attention_kv8_kernel<.., ROW>) or ONE split-context form (form = 2 / 3, chunk = 128 / 256: pass_kv8_split_kernel + prompt_merge_kernel).
struct PassAttention { int form, chunk, nsp, nsp_of_bin; };
bool pass_attention_plan(const Config* p, const RunState* s, int pos, int n, PassAttention* out);
// Positions pos0 = *s->pos .. + n - 1 (2 <= n <= PROMPT_PASS_MAX, all inside one bin and below the bound of q4_set_pass_context, all prompt-only) on the
// launch stream: K / V rows of every layer, then RunState::x, the device position and SharedData::pos as n per-token prompt steps leave them. No
// classifier, no sampler.
// With log-probability records on (admitted only with q4_set_pass_logprobs on): behind the layer loop the verify pass's classifier (spec_verify.h) over the
// n residual rows, the row form of the record launch (q4_logprobs.hip; the target of row r is the ring's tokens[pos0 + r + 1]) and a copy of the last row
// to RunState::logits -- records pos0 .. pos0 + n - 1 and the logits are what n prompt steps with records leave, byte for byte -- then the finish launch.
// sampler (q4_set_pass_stages admits the pass with the guide or the adaptive truncation on): what a prompt group of steps does in front of its launches --
// the guide's state ring and, where the sampler has the adaptive launch on and the model has the rings, Mirostat's mu ring put to NONE at pos0 .. pos0 + n - 1.
int run_prompt_pass(const Config* p, RunState* s, const TransformerWeights* w, Model* m, int pos0, int n, const Sampler* sampler = nullptr);
void pass_release(Model* m);   // q4_free_transformer: the scratch of this model's prompt and verify passes (Model::pass)
// q4_passes.hip. A prompt pass in place of the token loop's per-token prompt steps from `pos`: how many positions it takes, 0 for none (its comment there)
int prompt_pass_tokens(const Transformer* t, const Model* m, const Sampler* sampler, int pos, int num_prompt_tokens, int steps, int off);
// What the verify pass (spec_verify.h) shares with the prompt pass: the model's scratch rows -- Model::pass.x [PROMPT_PASS_MAX][dim] residual streams, .pos
// [PROMPT_PASS_MAX] their positions (prompt_pass_rows allocates the scratch on first use) -- and the layer loop over rows 0 .. n - 1 of them: the five launches per layer of
// run_prompt_pass (six in the split-context bins: the records' merge is a launch of its own), which reads the device position and moves nothing. The
// caller fills x and pos in front and takes the final residual streams from x.
int prompt_pass_rows(Model* m, const Config* p);
// Model::pass.logit_rows ([PROMPT_PASS_MAX][vocab] logits and the PROMPT_PASS_MAX tokens behind them) and Model::pass.lp_side ([PROMPT_PASS_MAX][vocab]
// raw rows of a pass under the sampler with records), each allocated on first use and released by pass_release
int pass_logit_rows(Model* m, const Config* p);
int pass_side_rows(Model* m, const Config* p);
int pass_draft_view(Model* m, const Config* p);   // Model::pass.view, [seq_len] ints: the draft view of a verify pass with logit stages (spec_verify.h)
int prompt_pass_layers(const Config* p, RunState* s, const TransformerWeights* w, Model* m, int pos0, int n);
// A scratch that is not a model's (the batch's, q4_batch.h): the rows of prompt_pass_rows in *b; the split passes' records grown to `floats` (synchronises
// where an older area may still be read); what pass_release does for a model's
int pass_scratch_rows(PassScratch* b, const Config* p);
int pass_records_of(PassScratch* b, size_t floats);
void pass_scratch_release(PassScratch* b);
// The rows one launch of a batch pass runs, by value in its arguments: n rows of the pass, row[i] their indices; nsp_of_bin[i] (the merge launch): the chunk
// count the step merges at row i's position, 0: those up to the position itself (PassAttention::nsp_of_bin)
struct PassRowList { int n; int row[PROMPT_PASS_MAX]; int nsp_of_bin[PROMPT_PASS_MAX]; };
// ... and, for the split launch's run form, beside a PassRowList of the runs' first rows: len[i] adjacent rows of one sequence from row[i] on
struct PassRunList { int len[PROMPT_PASS_MAX]; };
// The batch pass's side of this file (q4_batch.h): its admission by shape, and the layer loop over n rows of different sequences (their comments there)
bool batch_pass_covers(const Config* p, const Model* m);
int batch_pass_layers(const Config* p, const RunState* s, const TransformerWeights* w, Model* m, PassScratch* b, const int* pos_host, int n, q4_half* const* kv,
                      const int* seq);

}  // namespace q4
