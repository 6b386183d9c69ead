// q4_model.h -- what the library keeps beside a Transformer, what the host side's translation units (q4_model.hip, q4_network.hip, q4_step.hip,
// q4_sequence.hip, q4_passes.hip, q4_loops.hip) share, and the row a logit stage gives the step (not part of the C ABI).
#pragma once
#include <stddef.h>
#include <map>
#include <vector>
#include "q4_internal.h"
#include "cls_screen.h"

namespace q4 {

// The scratch of the prompt and verify passes (prompt_pass.h, spec_verify.h), each allocation made on first use and released by pass_release. slab: the rows x / q / xb
// / hb, their positions and the attention launch's sink (u32x2v granules); records: the split passes' flash-decode records; logit_rows: the logits of a verify pass or of a
// prompt pass with records (pass_logit_rows) and the tokens behind them; lp_side: [PROMPT_PASS_MAX][vocab] raw rows of a verify pass under the sampler with records (pass_side_rows);
// kv_stage: [2][PROMPT_PASS_MAX][kv_dim] the fp16 K and V staging rows of a pass over the FP8 cache (prompt_pass_kv8.h; q4_set_pass_kv8);
// view: [seq_len] the draft view of a verify pass with logit stages (pass_draft_view; q4_set_pass_stages): tokens by absolute position, the ring up to the pass's first position and its drafts behind
struct PassScratch { void* slab; q4_half* x; q4_half* q; q4_half* xb; q4_half* hb; int* pos; unsigned* sink; size_t sink_stride; float* records; size_t record_floats; q4_half* logit_rows; q4_half* lp_side; int* view; q4_half* kv_stage; };
// every Transformer owns two HBM slabs (weights, run state) instead of ~750 small allocations: layers sit
// back to back in HBM in the order the token loop streams them. ONE record per model: q4_build_transformer registers it as soon as its
// first allocation exists, q4_free_transformer is the only place that releases and forgets it.
struct Model {
    void* weights = nullptr;
    void* state = nullptr;
    void* shared = nullptr;
    void* logits_array = nullptr;
    float2* rope_table = nullptr;   // [seq_len][head_size/2] (cos, sin), lives exactly as long as the Transformer
    q4_rope_scaling rope = {};      // fixed at build time (q4_set_rope_scaling). kind Q4_ROPE_NONE: the table comes from rope_theta (rope_angle) and the two arrays below are empty;
    std::vector<float> inv_freq;    // else [head_size/2] frequencies (q4_rope_inv_freq), the table comes from them (rope_angle_freq) and is mandatory,
    float* inv_freq_dev = nullptr;  // and their device copy, which fusion level 0's rotation launch reads. rope.inv_freq is not kept: q4_rope_scaling_of points it at inv_freq
    unsigned* sync = nullptr;       // hand-off words of the attention -> o-proj launch (layout: q4_internal.h SYNC_*), null: the five-launch sequence
    size_t sync_words = 0;          // word 0 is the sticky error flag
    size_t att_bytes = 0;           // bytes of RunState::att (the split-context records live there)
    int kv_format = Q4_KV_FP16;     // fixed at build time (q4_set_kv_format). Q4_KV_FP8: RunState::key_cache / value_cache point at [layer][seq_len][kv_dim] e4m3 BYTES, and
    int8_t* k_exp = nullptr;        // [layer][n_kv_heads][seq_len] row exponents (contiguous per head: a chunk reads a run of bytes),
    int8_t* v_exp = nullptr;
    q4_half* k_row = nullptr;       // [kv_dim] fp16 staging rows: the current position's K (rotated) and V between the QKV launch and the attention launch that appends them
    q4_half* v_row = nullptr;       // (all four live in the state slab, behind RunState's buffers -- RunState's layout is ABI -- and are zeroed with it)
    double kv_price = 0.0;          // 10 ns ticks per context position of this model's K / V stream on this device (measure_kv_price), 0.0: not measured
    int logprobs_k = -1;            // q4_set_logprobs: -1 off, else the K of the record ring below (one allocation, lp_ring, carved into arrays by position)
    void* lp_ring = nullptr;
    float* lp_lse = nullptr;        // [seq_len]
    float* lp_token = nullptr;      // [seq_len] token_logprob
    int* lp_ids = nullptr;          // [seq_len][K]
    float* lp_top = nullptr;        // [seq_len][K]
    q4_half* lp_side = nullptr;     // [vocab] raw logits of a sampled step, kept for the look-up behind the sampler
    bool pass_logprobs = false;     // q4_set_pass_logprobs: prompt and verify passes (and q4_score_ids through prompt passes) also while the records are on
    bool pass_gqa = false;          // q4_set_pass_gqa: prompt and verify passes also for the grouped-query 4096-wide shape (prompt_pass_covers)
    bool pass_kv8 = false;          // q4_set_pass_kv8: prompt and verify passes also for a model with the FP8 cache (prompt_pass_covers; prompt_pass_kv8.h)
    bool pass_13b = false;          // q4_set_pass_13b: prompt and verify passes also for Llama-2-13B's shape, dim 5120 / hidden 13824 (prompt_pass_covers)
    bool pass_stages = false;       // q4_set_pass_stages: verify passes also with a guide, DRY or the sampling controls on (their row forms), prompt passes also with a guide or the adaptive truncation on
    ClsScreen screen;               // the int8 screening copy of wcls (cls_screen.h), base null: none -- the shape has no strips form, or the allocation failed
    const q4_guide* guide = nullptr;   // q4_set_guide: null off. The ring and the block are allocated with the model's first guide and live as long as the model
    int* guide_state = nullptr;     // [guide_len = seq_len] the automaton's state by position (Q4_GUIDE_NONE / Q4_GUIDE_OFFTRACK)
    int guide_len = 0;
    void* guide_block = nullptr;    // what the guide launch reads: {table, ring, sizes}; captured graphs hold its address
    float* adaptive_mu = nullptr;   // q4_sampler_set_adaptive: ONE allocation made by the first step that runs the launch with this model, kept until q4_free_transformer --
    float* adaptive_rec = nullptr;  // Mirostat's mu by position [adaptive_len = seq_len] (every byte 0xFF, a NaN: none), the records [adaptive_len][Q4_ADAPTIVE_RECORD]
    float* adaptive_side = nullptr; // and the side buffer [vocab + 2]: the kept entries' w of the last launch, {side_pos (an int), side_lse}
    int adaptive_len = 0;
    unsigned long long fingerprint = 0;   // of the checkpoint file (q4_build_transformer): the header without seq_len, the file's size, its first and last 64 KiB; what a snapshot is matched by
    int shift_keep = 0, shift_discard = 0;   // q4_set_context_shift: what the library's own token loops shift by at seq_len; discard 0: off
    int shifted_keep = -1;          // the smallest n_keep of the q4_shift_context calls since the last q4_reset_sequence, -1: none -- rows above it are not "computed from the ring's tokens" (q4_common_prefix)
    int spec_draft = 0, spec_ngram_max = 0, spec_ngram_min = 0;   // q4_set_speculative: the most drafts a verify pass of the token loops carries (0: off) and the built-in drafter's n-gram range
    bool spec_sampled = false;      // q4_set_speculative_sampled: verify passes also under a temperature / top-p sampler (each row sampled with its position's coin)
    q4_drafter_fn drafter = nullptr;  // q4_set_drafter: null, the built-in drafter (q4_spec_draft)
    void* drafter_ctx = nullptr;
    long long spec_passes = 0, spec_drafted = 0, spec_accepted = 0;   // q4_spec_stats
    long long forced_drafted = 0, forced_accepted = 0;                // q4_spec_stats_forced: of those, the drafts the guide's forced run gave and how many were accepted
    PassScratch pass = {};          // nothing until the model's first prompt or verify pass
    bool rows_suspect = false;      // q4_handoff_status reported a time-out and no q4_reset_sequence has followed: the K / V rows below the position are not to be reused (q4_common_prefix)
};
// the network entry points take (Config, RunState, TransformerWeights), not the Transformer: the record is found by RunState (&t->state)
using Models = std::map<const RunState*, Model>;
Models& models();
// null for a RunState the library did not build (the public per-kernel API): no table, no hand-off words, the five-launch sequence
static inline Model* model_of(const RunState* s) {
    auto it = models().find(s);
    return it == models().end() ? nullptr : &it->second;
}

// The Transformer around a RunState / a Config that model_of has said the library built: both sit inside it
static inline const Transformer* transformer_of(const RunState* s) { return reinterpret_cast<const Transformer*>(reinterpret_cast<const char*>(s) - offsetof(Transformer, state)); }
static inline const Transformer* transformer_of(const Config* p) { return reinterpret_cast<const Transformer*>(reinterpret_cast<const char*>(p) - offsetof(Transformer, config)); }
#define Q4_TRY(call) do { int rc__ = (call); if (rc__) return rc__; } while (0)

// q4_model.hip: the process-wide setting q4_build_transformer reads (q4_set_rope_scaling); its inv_freq points at the library's copy
extern q4_rope_scaling g_rope_scaling;

// q4_network.hip. have_embedding: the preceding launch of the stream (the greedy sampler of the previous step, inside one graph replay) has left
// the token's embedding row in s->x already
// screened: the classifier as screen + refine (cls_screen.h): RunState::logits then holds the exact logits of the rows that can be the largest and -inf elsewhere
int run_network(const int* pPos, const Config* p, RunState* s, const TransformerWeights* w, int seq_len_bin, bool have_embedding, bool screened = false);
// q4_step.hip
void drop_graphs_of(const RunState* s);   // the model's captured graphs, after the launch stream has drained
void drop_logprob_graphs_of(const RunState* s);   // ... those that contain the log-probability launch only
bool any_stage_on(const Sampler* sampler, const Model* m);        // a logit stage of the table below is on for this sampler and model
bool stages_take_rows(const Sampler* sampler, const Model* m);    // ... and every stage that is on has a row form (LogitStage::launch_rows)
// The stages that are on, in table order, over the n_rows logit rows of a verify pass (`ld` halves apart): prepare (never inside a capture: no graph holds a
// pass), then the row form. view: the pass's draft view, pos_rows: the rows' positions (both device). Q4_ERR_ARG where a stage that is on has no row form
int launch_stage_rows(const Sampler* sampler, Model* m, const Config* p, q4_half* rows, int ld, int n_rows, const int* view, const int* pos_rows);
int stages_clear_positions(const Sampler* sampler, const Model* m, int pos, int n);   // a prompt pass's positions: state by position to NONE, as a prompt group of steps does
int graph_bin(int seq_len, const Config* p, int* seq_len_bin_out);   // the graph bin of a step whose sequence length is seq_len: its index, and its size
// q4_logprobs.hip. The record launch of a step (in front of the sampler: reads the position before it advances) and the chosen token's look-up behind
// the sampler of a sampled step
// ... and of a pass with q4_set_pass_logprobs on: the row form of both, one block per row of the pass's logits (their comments there). The modes of the
// record launch: the target is the ring's next token (prompt steps), entry 0 (greedy generating steps), or looked up behind the sampler
enum { LP_TARGET = 0, LP_GREEDY = 1, LP_SAMPLED = 2 };
bool logprobs_size_ok(int n, int top_k);
int launch_logprobs_step(const Model* m, const Config* p, RunState* s, int gen_token, bool greedy);
int launch_logprobs_pick(const Model* m, const Config* p, RunState* s);
int launch_logprobs_rows(const Model* m, const Config* p, RunState* s, const q4_half* rows, int ld, int n, int mode);
int launch_logprobs_pick_rows(const Model* m, const Config* p, RunState* s, int n, const int* win);
// A logit stage: ONE launch that rewrites a generating step's fp16 logits in place, between the record launch and the argmax / sampler. What it reads
// sits in a small device block whose address -- and nothing else of the stage -- a captured graph holds. m is null for a RunState the
// library did not build.
struct LogitStage {
    bool (*on)(const Sampler* sampler, const Model* m);
    // in front of a step, outside any capture: the settings against this model, the block (allocated once, rewritten in stream order when the host
    // changed a value), and whatever else the launch needs allocated. An error refuses the step
    int (*prepare)(const Sampler* sampler, Model* m, const Config* p, const void** block);
    int (*launch)(const void* block, const Model* m, const Config* p, RunState* s);
    // per-Sampler stages: the block a Sampler owns (null: none yet; never creates one), and what destroy_sampler calls once the graphs that hold
    // that block are gone and the stream has drained. Both null for a stage that lives with the model
    const void* (*block)(const Sampler* sampler);
    void (*forget)(const Sampler* sampler);
    // The row form, for a verify pass with q4_set_pass_stages on: block r of n_rows <= PROMPT_PASS_MAX rewrites rows + r * ld at position pos_rows[r] and reads
    // its tokens from the draft view (device, by absolute position) instead of the pinned ring; what row r receives is byte for byte what `launch` writes for
    // that row alone at that position. Null: the stage has no row form and a pass is not admitted while it is on (the adaptive truncation)
    int (*launch_rows)(const void* block, const Model* m, const Config* p, q4_half* rows, int ld, int n_rows, const int* view, const int* pos_rows);
};
// q4_step.hip's table, in launch order: the guide's mask (q4_guide.hip; per model), DRY (q4_dry.hip), the sampling controls (q4_logit_process.hip:
// top-k counts what both left), the adaptive truncation (q4_adaptive.hip: typical-p and Mirostat see what top-k and min-p left)
// (Written once, where they are defined. Not const: a const object with a constant initializer is emitted for the device as well, where these host
// functions do not exist.)
extern LogitStage guide_stage, dry_stage, controls_stage, adaptive_stage;
// q4_adaptive.hip. NONE over the ring positions of a prompt group or over the whole ring (in stream order, outside any capture; nothing without
// rings); the move of q4_shift_context; what q4_free_transformer releases
int adaptive_clear_positions(const Model* m, int pos, int nsteps);
int adaptive_clear_ring(const Model* m);
int adaptive_shift(const Model* m, int vocab, int n_pos, int first, int M, int D);
void adaptive_release(Model* m);
// q4_guide.hip. NONE over the ring positions of a prompt group, or over the whole ring (both in stream order, outside any capture); what
// q4_free_transformer releases
int guide_clear_positions(const Model* m, int pos, int nsteps);
int guide_clear_ring(const Model* m);
void guide_release(Model* m);
// The token loop's forced drafts (q4_set_pass_stages; the device has published position `pos`, so the guide launch of the step in front has run): the state
// behind ring[pos] -- state[pos - 1] read back with one 4-byte copy (NONE at pos 0), then the kernel's rule 2 on the host, its table entry one 2-byte copy --
// and from it q4_guide_forced_run's tokens, at most max_draft, into draft; *n_out how many
int guide_forced_draft(const Model* m, const int* ring, int pos, int max_draft, int* draft, int* n_out);
// q4_kv_copy.hip. One launch that copies up to KV_COPY_MAX_RUNS strided runs on the launch stream: run r of an entry moves run_bytes bytes from
// src + r * src_stride to dst + r * dst_stride, r < outer. Q4_ERR_ARG without a launch: a null pointer, a negative field, run_bytes above a stride when
// outer > 1, source and destination ranges that overlap
enum { KV_COPY_MAX_RUNS = 4 };
struct CopyRun { void* dst; const void* src; long long outer, dst_stride, src_stride, run_bytes; };
int copy_runs_check(const CopyRun& c);
int launch_copy_runs(const CopyRun* runs, int n);
// q4_kv_shift.hip. One in-place launch on the launch stream: rows [n_keep + n_discard, n_pos) of every layer move down by n_discard, K rows rotated by
// cos_sin ([head_size/2] (cos, sin) pairs on the device). The argument checks of q4_kv_shift (llama2_q4.h); n_pos == n_keep + n_discard launches nothing
int launch_kv_shift(void* k, void* v, int8_t* k_exp, int8_t* v_exp, int kv_format, int n_layers, int seq_len, int n_kv_heads, int head_size, int n_pos,
                    int n_keep, int n_discard, const float* cos_sin);

}  // namespace q4
