// q4_step.hip -- one decode step: the table of logit stages, per-model graph sets and q4_run_transformer*, the sampler's host side with the coin ring (captured graphs bake
// their addresses). Between steps: q4_sequence.hip; over them: q4_passes.hip, q4_loops.hip. Mirrors llama2_q4.cu:342-395 (run_transformer), sampler.h.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stdlib.h>
#include <string.h>
#include "q4_model.h"
#include "q4_loop.h"
#include "spec_verify.h"

namespace q4 {

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
bool any_stage_on(const Sampler* sampler, const Model* m) {
    for (const LogitStage* st : STAGES)
        if (st->on(sampler, m)) return true;
    return false;
}
bool stages_take_rows(const Sampler* sampler, const Model* m) {
    bool any = false;
    for (const LogitStage* st : STAGES)
        if (st->on(sampler, m)) {
            if (!st->launch_rows) return false;
            any = true;
        }
    return any;
}
int launch_stage_rows(const Sampler* sampler, Model* m, const Config* p, q4_half* rows, int ld, int n_rows, const int* view, const int* pos_rows) {
    for (const LogitStage* st : STAGES)
        if (st->on(sampler, m)) {
            const void* block = nullptr;
            if (!st->launch_rows) return Q4_ERR_ARG;
            Q4_TRY(st->prepare(sampler, m, p, &block));
            Q4_TRY(st->launch_rows(block, m, p, rows, ld, n_rows, view, pos_rows));
        }
    return Q4_OK;
}
// What a prompt group does to state by position in front of its launches (run_transformer_steps_screenable below), for a prompt pass: the guide's ring
// while the model has a guide, Mirostat's while the sampler has the adaptive launch on and the model has the rings, to NONE over [pos, pos + n)
int stages_clear_positions(const Sampler* sampler, const Model* m, int pos, int n) {
    if (guide_stage.on(sampler, m)) Q4_TRY(guide_clear_positions(m, pos, n));
    if (m && m->adaptive_mu && adaptive_stage.on(sampler, m)) Q4_TRY(adaptive_clear_positions(m, pos, n));
    return Q4_OK;
}
static bool step_screens(const Model* m, bool may_screen, int gen_token, bool greedy, int copyLogits, const Sampler* sampler) {
    return may_screen && g_greedy_screen && gen_token && greedy && !copyLogits && g_fusion >= 1 && m && m->logprobs_k < 0 && m->screen.base &&
           !any_stage_on(sampler, m) && cls_screen_shape(m->screen.n, m->screen.d);
}

// The graph bin of a step whose sequence length is seq_len (llama2_q4.cu:355-360): the index of its graph set and the bin's size
int graph_bin(int seq_len, const Config* p, int* seq_len_bin_out) {
    int graphIndex;
    int seq_len_bin = 128;
    for (graphIndex = 0; graphIndex < Q4_MAX_GRAPHS - 1; seq_len_bin *= 2, graphIndex++)
        if (seq_len <= seq_len_bin) break;                                         // :356-359
    if ((seq_len > seq_len_bin) || (graphIndex == Q4_MAX_GRAPHS - 1)) seq_len_bin = p->seq_len;   // :360
    *seq_len_bin_out = seq_len_bin;
    return graphIndex;
}

}  // namespace q4

using namespace q4;

extern "C" __attribute__((visibility("hidden"))) int q4_copy_logits_at_pos(float* logits_array, const q4_half* logits, int vocab_size, const int* pPos);

extern "C" {

// The greedy steps' classifier as an int8 screen + exact refinement (cls_screen.h). 1 (default): on, for models that have a screening copy; 0: off.
void q4_set_greedy_screen(int on) {
    g_greedy_screen = on ? 1 : 0;
    q4_reset_graphs();
}
int q4_get_greedy_screen(void) { return g_greedy_screen; }

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
}  // extern "C"
int q4::stage_pass_coins(Sampler* sampler, const Config* p, int pos, int n_draft, const float** coins_dev) {
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
extern "C" {
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
// ... for the token loops of this library (q4_loops.hip's q4_token_loop, q4_chat; q4_loop.h): may_screen says that nobody reads the group's logits
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
    if (pos + k == steps && gen0 && sampler && sampler->temperature == 0.0f && step_screens(model_of(&transformer_of(p)->state), true, 1, true, 0, sampler)) return 1;
    return k;
}

}  // extern "C"
