// q4_batch.hip -- batched decoding (q4_batch.h): the batch object, its scheduler and its three small launches. A pass is
//   1. batch_embed_kernel: row r <- the embedding of ring[slot][pos + off] for (slot, off) = (map.slot[r], map.off[r]), the rows' positions and cache bases for the layers;
//   2. batch_pass_layers (prompt_pass.hip): the pass layer loop in its row forms (split-context attention of a slot's several rows: the run form);
//   3. the verify pass's classifier (spec_verify.hip) over each slot's LAST row -- gathered first (batch_gather_kernel) when a slot carries several --,
//      under a sampler the row form of its two launches (q4_sampling.hip);
//   4. batch_pick_kernel: per slot the step's argmax (or the sampler's token), the slot's logits row, its next ring entry and its position.
// Every dependency is a launch boundary on the q4 stream: no launch waits, polls or uses an atomic, and a slot's words have one writer per launch.
// Which slot takes how many rows is q4_batch_plan_rows' schedule: one per open slot and, with q4_batch_set_prefill above 1, the spare rows to slots inside
// their prompts as consecutive positions. A row at position p + 1 attends over the K / V row its slot's row at p wrote in the same pass's q/k/v launch.
// The host never reads a position back to plan a pass: a slot advances by its planned row count, so its position -- and with it each row's attention
// form -- is known on the host; the kernels take the positions from the device words all the same. Not in the reference (one sequence, one step per token).
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>
#include <new>
#include <vector>
#include "q4_device.h"
#include "q4_batch.h"
#include "spec_verify.h"
using namespace q4;

namespace {

// the batch's words on the device: by slot, and -- rewritten by every pass's first launch -- by row
struct BatchWords {
    int pos[BATCH_MAX_SLOTS];            // the slot's position: the ring entry its next row carries
    int n_prompt[BATCH_MAX_SLOTS];       // ring[0 .. n_prompt) is given; the pass at n_prompt - 1 generates the first token
    int out[BATCH_MAX_SLOTS];            // q4_batch_step's tokens_out of the last pass
    q4_half* kv[2 * BATCH_MAX_SLOTS];    // by row: the cache bases of the row's slot, K then V (GemvArgs::row_kv)
    float coin[BATCH_MAX_SLOTS];         // by row: the coin of the row's slot at its position
    int win[BATCH_MAX_SLOTS];            // by row: the token the row form of the sampler chose
};

}  // namespace

struct q4_batch {
    Transformer* t = nullptr;
    int n_slots = 0;
    size_t cache_halves = 0;             // of one slot's K (= V) cache: n_layers * seq_len * kv_dim
    q4_half* k = nullptr;                // [n_slots][cache_halves]
    q4_half* v = nullptr;
    int* ring = nullptr;                 // [n_slots][seq_len + 1]
    q4_half* logits = nullptr;           // [n_slots][vocab]: a slot's last position
    q4_half* rows = nullptr;             // [BATCH_MAX_SLOTS][vocab]: the classifier's rows of a pass
    BatchWords* words = nullptr;
    int* log = nullptr;                  // q4_batch_generate's [log_passes][BATCH_MAX_SLOTS] tokens
    int log_passes = 0;
    PassScratch scratch = {};
    // what the host knows without asking: a slot moves only through this file. The device words move in a pass's LAST launch, the host's once all of its
    // launches are queued: a pass that fails half-way with Q4_ERR_HIP leaves the two apart -- the batch is then dead: delete it.
    bool open[BATCH_MAX_SLOTS] = {};
    int pos[BATCH_MAX_SLOTS] = {};
    int n_prompt[BATCH_MAX_SLOTS] = {};
    int prefill = 1;                     // q4_batch_set_prefill: the most rows one slot takes in a pass
    unsigned long long rng[BATCH_MAX_SLOTS] = {};
};

namespace {

// the rows of a pass: embeddings from each slot's pending token; the positions and cache bases the layer launches read by row; the coins
__global__ void batch_embed_kernel(q4_half* xs, const q4_half* table, int dim, const BatchRowMap map, BatchWords* w, const int* ring, int ring_stride,
                                   q4_half* k, q4_half* v, size_t cache_halves, int* pos_rows) {
    const int u = blockIdx.x * blockDim.x + threadIdx.x, r = blockIdx.y;
    const int slot = map.slot[r];
    const int pos = w->pos[slot] + map.off[r];
    if (u == 0) {
        pos_rows[r] = pos;
        w->kv[r] = k + (size_t)slot * cache_halves;
        w->kv[BATCH_MAX_SLOTS + r] = v + (size_t)slot * cache_halves;
        if (r < map.m) w->coin[r] = map.coin[r];            // (by slot of the pass, for the sampler's rows: block r is its only writer)
    }
    if (u >= (dim >> 3)) return;
    const int token = ring[(size_t)slot * ring_stride + pos];
    reinterpret_cast<u32x4*>(xs + (size_t)r * dim)[u] = reinterpret_cast<const u32x4*>(table + (size_t)token * dim)[u];
}

// One block per slot of the pass, on the classifier's row r of that slot's last row (map.last[r]; the slot's earlier rows of the pass are prompt rows
// whose tokens a prompt step discards: nobody computes them). The row's token: argmax_kernel's rule (q4_kernels.hip; verify_accept_kernel restates it the same way) -- 16-byte loads, the first
// maximum inside a thread, value then lower index across threads, 0 for a row without a finite or +inf entry -- or, GIVEN, what the row form of the sampler
// left in win[r] (the row then holds fp16 probabilities, which is what a sampled step leaves in RunState::logits). Then what the step leaves for this
// sequence: the logits row, ring[pos + cnt] unless that entry is still a prompt token (the computed token is discarded, as a prompt step's), the position
// advanced by the slot's cnt rows.
// log: where this pass's tokens_out go ([BATCH_MAX_SLOTS] by slot; the host has put -1 into the others).
template <bool GIVEN>
__global__ void __launch_bounds__(1024) batch_pick_kernel(const q4_half* rows, const int size, const BatchRowMap map, BatchWords* w, int* ring, int ring_stride,
                                                          q4_half* logits, int* log) {
    __shared__ float sval[16];
    __shared__ int sidx[16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = blockIdx.x;
    const int slot = map.slot[map.last[r]];
    const int n8 = size >> 3;                                // (the vocabulary is a multiple of 8: verify_cls_covers)
    const q4_half* row = rows + (size_t)r * size;
    q4_half* keep = logits + (size_t)slot * size;
    float max_val = -INFINITY;
    int max_pos = 0x7fffffff;
    for (int u = tid; u < n8; u += blockDim.x) {
        const u32x4 v = reinterpret_cast<const u32x4*>(row)[u];
        reinterpret_cast<u32x4*>(keep)[u] = v;
        if (GIVEN) continue;
#pragma unroll
        for (int e = 0; e < 4; e++) {
            const h2 p = as_h2(v[e]);
            const float a = (float)p.x, b = (float)p.y;
            if (a > max_val) { max_val = a; max_pos = u * 8 + 2 * e; }
            if (b > max_val) { max_val = b; max_pos = u * 8 + 2 * e + 1; }
        }
    }
    if (!GIVEN) {
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const float ov = __shfl_xor(max_val, off);
            const int op = __shfl_xor(max_pos, off);
            if (ov > max_val || (ov == max_val && op < max_pos)) { max_val = ov; max_pos = op; }
        }
        if (lane == 0) { sval[wave] = max_val; sidx[wave] = max_pos; }
        __syncthreads();
    }
    if (tid == 0) {
        int token;
        if (GIVEN) {
            token = w->win[r];
        } else {
            const int nw = blockDim.x >> 6;
            for (int i = 1; i < nw; i++)
                if (sval[i] > max_val || (sval[i] == max_val && sidx[i] < max_pos)) { max_val = sval[i]; max_pos = sidx[i]; }
            token = max_pos == 0x7fffffff ? 0 : max_pos;     // all NaN / -inf
        }
        const int next = w->pos[slot] + map.cnt[r];          // the slot's rows of this pass were positions pos .. next - 1, this one the last
        const bool gen = next >= w->n_prompt[slot];
        if (gen) ring[(size_t)slot * ring_stride + next] = token;
        log[slot] = gen ? token : -1;
        w->pos[slot] = next;
    }
}

// A pass in which a slot carries several rows: the residual streams of the slots' last rows, gathered into map.m contiguous rows for the classifier
__global__ void batch_gather_kernel(q4_half* dst, const q4_half* xs, int dim, const BatchRowMap map) {
    const int u = blockIdx.x * blockDim.x + threadIdx.x, j = blockIdx.y;
    if (u >= (dim >> 3)) return;
    reinterpret_cast<u32x4*>(dst + (size_t)j * dim)[u] = reinterpret_cast<const u32x4*>(xs + (size_t)map.last[j] * dim)[u];
}

// a slot's words when it opens; -1 into a pass's tokens_out
__global__ void batch_slot_kernel(BatchWords* w, int slot, int pos, int n_prompt) {
    w->pos[slot] = pos;
    w->n_prompt[slot] = n_prompt;
}
__global__ void batch_log_clear_kernel(int* log) { log[threadIdx.x] = -1; }

void release(q4_batch* b) {
    for (void* d : {(void*)b->k, (void*)b->v, (void*)b->ring, (void*)b->logits, (void*)b->rows, (void*)b->words, (void*)b->log})
        if (d) (void)hipFree(d);
    pass_scratch_release(&b->scratch);
    delete b;
}

Model* model(const q4_batch* b) { return b && b->t ? model_of(&b->t->state) : nullptr; }
bool slot_ok(const q4_batch* b, int slot) { return b && slot >= 0 && slot < b->n_slots; }

// what a batch cannot run beside: the model's switches that a later call may have turned on, and the sampler's
int step_admitted(const q4_batch* b, const Model* m, const Sampler* sampler) {
    const Config* p = &b->t->config;
    if (g_fusion < 3 || !batch_pass_covers(p, m) || m->guide || m->logprobs_k >= 0 || any_stage_on(sampler, m)) return Q4_ERR_UNSUPPORTED_SIZE;
    if (sampler->temperature != 0.0f && (sampler->vocab_size != p->vocab_size || !sample_rows_covers(sampler))) return Q4_ERR_UNSUPPORTED_SIZE;
    return Q4_OK;
}

// One pass, queued: log (device, [BATCH_MAX_SLOTS]) receives its tokens_out. The caller has checked the admission and that no open slot stands at seq_len.
int queue_pass(q4_batch* b, Model* m, Sampler* sampler, int* log) {
    const Config* p = &b->t->config;
    const TransformerWeights* w = &b->t->weights;
    const int dim = p->dim, vocab = p->vocab_size, ring_stride = p->seq_len + 1;
    const bool sampled = sampler->temperature != 0.0f;
    if (sampled) Q4_TRY(sample_rows_prepare(sampler));      // (scratch on first use and the LDS opt-in: in front of the pass's first launch)
    BatchRowMap map = {};
    int pos_rows[BATCH_MAX_SLOTS], seq[BATCH_MAX_SLOTS], count[BATCH_MAX_SLOTS], open[BATCH_MAX_SLOTS];
    unsigned long long rng[BATCH_MAX_SLOTS];                 // by slot of the pass: the coin streams behind this pass, the slots' once the pass is queued
    for (int s = 0; s < b->n_slots; s++) open[s] = b->open[s] ? 1 : 0;
    if (q4_batch_plan_rows(open, b->pos, b->n_prompt, b->n_slots, b->prefill, count) < 0) return Q4_ERR_ARG;
    for (int s = 0; s < b->n_slots; s++) {
        if (!count[s]) continue;
        const int j = map.m++;
        rng[j] = b->rng[s];
        for (int i = 0; i < count[s]; i++) {
            map.coin[j] = random_f32(&rng[j]);               // one coin per position, drawn whether or not the pass samples (q4_generate_ids' rule): the last row's stays
            map.slot[map.n] = s;
            map.off[map.n] = i;
            seq[map.n] = s;
            pos_rows[map.n++] = b->pos[s] + i;
        }
        map.last[j] = map.n - 1;
        map.cnt[j] = count[s];
    }
    // every row's attention as the step at its position would run it: a position whose step form no pass restates (without graphs: the one-block form at
    // 256 .. 510) refuses the whole pass in front of its first launch
    for (int r = 0; r < map.n; r++) {
        PassAttention plan;
        if (!pass_attention_plan(p, &b->t->state, pos_rows[r], 1, &plan)) return Q4_ERR_UNSUPPORTED_SIZE;
    }
    Q4_LAUNCH(batch_log_clear_kernel, dim3(1), dim3(BATCH_MAX_SLOTS), 0, log);
    Q4_LAUNCH_CHECK();
    if (!map.n) return Q4_OK;
    const PassScratch* sc = &b->scratch;
    Q4_LAUNCH(batch_embed_kernel, dim3(divUp(dim >> 3, 256), map.n), dim3(256), 0, sc->x, w->token_embedding_table, dim, map, b->words, (const int*)b->ring, ring_stride,
              b->k, b->v, b->cache_halves, sc->pos);
    Q4_LAUNCH_CHECK();
    const bool several = map.n > map.m;                      // some slot carries more than one row
    Q4_TRY(batch_pass_layers(p, &b->t->state, w, m, &b->scratch, pos_rows, map.n, b->words->kv, several ? seq : nullptr));
    // the classifier only where a token or a slot's logits row needs it -- every slot's last row: those rows' residual streams gathered into sc->q (free
    // behind the layers); one row per slot: they are rows 0 .. n - 1 of sc->x as they stand
    const q4_half* last_x = sc->x;
    if (several) {
        Q4_LAUNCH(batch_gather_kernel, dim3(divUp(dim >> 3, 256), map.m), dim3(256), 0, sc->q, (const q4_half*)sc->x, dim, map);
        Q4_LAUNCH_CHECK();
        last_x = sc->q;
    }
    Q4_TRY(launch_verify_cls(b->rows, last_x, w->rms_final_weight, w->wcls, dim, vocab, map.m));
    if (sampled) {
        Q4_TRY(launch_sample_rows(sampler, b->rows, vocab, map.m, b->words->coin, nullptr, b->words->win));
        Q4_LAUNCH(batch_pick_kernel<true>, dim3(map.m), dim3(1024), 0, (const q4_half*)b->rows, vocab, map, b->words, b->ring, ring_stride, b->logits, log);
    } else {
        Q4_LAUNCH(batch_pick_kernel<false>, dim3(map.m), dim3(1024), 0, (const q4_half*)b->rows, vocab, map, b->words, b->ring, ring_stride, b->logits, log);
    }
    Q4_LAUNCH_CHECK();
    for (int j = 0; j < map.m; j++) { const int s = map.slot[map.last[j]]; b->pos[s] += map.cnt[j]; b->rng[s] = rng[j]; }
    return Q4_OK;
}

bool at_bound(const q4_batch* b) {
    for (int s = 0; s < b->n_slots; s++)
        if (b->open[s] && b->pos[s] >= b->t->config.seq_len) return true;
    return false;
}

// a closed slot opens at `pos` on prompt[0 .. n_prompt): the ring, the words, the coin stream behind `pos` draws
int open_slot(q4_batch* b, int slot, const int* prompt, int n_prompt, int pos, unsigned long long seed) {
    const int ring_stride = b->t->config.seq_len + 1;
    Q4_HIP(hipMemcpyAsync(b->ring + (size_t)slot * ring_stride, prompt, (size_t)n_prompt * sizeof(int), hipMemcpyHostToDevice, g_stream));   // (pageable: staged before the call returns)
    Q4_LAUNCH(batch_slot_kernel, dim3(1), dim3(1), 0, b->words, slot, pos, n_prompt);
    Q4_LAUNCH_CHECK();
    b->open[slot] = true;
    b->pos[slot] = pos;
    b->n_prompt[slot] = n_prompt;
    b->rng[slot] = seed;
    for (int i = 0; i < pos; i++) (void)random_f32(&b->rng[slot]);
    return Q4_OK;
}

int check_open(const q4_batch* b, int slot, const int* prompt, int n_prompt) {
    if (!slot_ok(b, slot) || b->open[slot] || !prompt || n_prompt < 1 || n_prompt > b->t->config.seq_len) return Q4_ERR_ARG;
    for (int i = 0; i < n_prompt; i++)
        if (prompt[i] < 0 || prompt[i] >= b->t->config.vocab_size) return Q4_ERR_ARG;
    return Q4_OK;
}

}  // namespace

extern "C" {

int q4_batch_covers(const Transformer* t) {
    const Model* m = t ? model_of(&t->state) : nullptr;
    return m && batch_pass_covers(&t->config, m) && !m->guide && m->logprobs_k < 0 ? 1 : 0;
}

int q4_batch_new(q4_batch** out, Transformer* t, int n_slots) {
    if (!out || !t || !model_of(&t->state) || n_slots < 1 || n_slots > BATCH_MAX_SLOTS) return Q4_ERR_ARG;
    if (!q4_batch_covers(t)) return Q4_ERR_UNSUPPORTED_SIZE;
    const Config* p = &t->config;
    q4_batch* b = new (std::nothrow) q4_batch();
    if (!b) return Q4_ERR_ALLOC;
    b->t = t;
    b->n_slots = n_slots;
    b->cache_halves = (size_t)p->n_layers * p->seq_len * ((size_t)p->dim / p->n_heads * p->n_kv_heads);
    const size_t cache = (size_t)n_slots * b->cache_halves * sizeof(q4_half), ring = (size_t)n_slots * (p->seq_len + 1) * sizeof(int);
    const size_t vocab = (size_t)p->vocab_size * sizeof(q4_half);
    int rc = Q4_OK;
    if (hipMalloc((void**)&b->k, cache) != hipSuccess || hipMalloc((void**)&b->v, cache) != hipSuccess || hipMalloc((void**)&b->ring, ring) != hipSuccess ||
        hipMalloc((void**)&b->logits, n_slots * vocab) != hipSuccess || hipMalloc((void**)&b->rows, BATCH_MAX_SLOTS * vocab) != hipSuccess ||
        hipMalloc((void**)&b->words, sizeof(BatchWords)) != hipSuccess) {
        (void)hipGetLastError();
        rc = Q4_ERR_ALLOC;
    }
    if (!rc) rc = pass_scratch_rows(&b->scratch, p);
    if (!rc && (hipMemsetAsync(b->k, 0, cache, g_stream) != hipSuccess || hipMemsetAsync(b->v, 0, cache, g_stream) != hipSuccess ||
                hipMemsetAsync(b->ring, 0, ring, g_stream) != hipSuccess || hipMemsetAsync(b->logits, 0, n_slots * vocab, g_stream) != hipSuccess ||
                hipMemsetAsync(b->words, 0, sizeof(BatchWords), g_stream) != hipSuccess || hipStreamSynchronize(g_stream) != hipSuccess))
        rc = Q4_ERR_HIP;
    if (rc) { release(b); return rc; }
    *out = b;
    return Q4_OK;
}

// The schedule of a pass, on the host alone (no HIP call): one row for every open slot first, so nobody starves; then the spare rows, in slot order, to
// the slots still in front of their last prompt position (pos < n_prompt - 1) -- each up to min(max_rows_per_slot, n_prompt - pos) rows in all, consecutive
// positions from pos, the last of them at most the generating row n_prompt - 1. A decoding slot never takes more than one: its next token does not exist yet.
int q4_batch_plan_rows(const int* open, const int* pos, const int* n_prompt, int n_slots, int max_rows_per_slot, int* rows_per_slot) {
    if (!open || !pos || !n_prompt || !rows_per_slot || n_slots < 1 || n_slots > BATCH_MAX_SLOTS || max_rows_per_slot < 1 || max_rows_per_slot > BATCH_MAX_SLOTS)
        return -Q4_ERR_ARG;
    int total = 0;
    for (int s = 0; s < n_slots; s++) total += rows_per_slot[s] = open[s] ? 1 : 0;
    for (int s = 0; s < n_slots && total < BATCH_MAX_SLOTS; s++) {
        if (!open[s] || pos[s] < 0 || pos[s] >= n_prompt[s] - 1) continue;
        const int left = n_prompt[s] - pos[s];
        int want = (left < max_rows_per_slot ? left : max_rows_per_slot) - 1;
        if (want > BATCH_MAX_SLOTS - total) want = BATCH_MAX_SLOTS - total;
        rows_per_slot[s] += want;
        total += want;
    }
    return total;
}

int q4_batch_set_prefill(q4_batch* b, int max_rows_per_slot) {
    if (!b || max_rows_per_slot < 1 || max_rows_per_slot > BATCH_MAX_SLOTS) return Q4_ERR_ARG;
    b->prefill = max_rows_per_slot;
    return Q4_OK;
}

int q4_batch_get_prefill(const q4_batch* b) { return b ? b->prefill : -Q4_ERR_ARG; }

int q4_batch_delete(q4_batch* b) {
    if (!b) return Q4_ERR_ARG;
    if (g_stream) Q4_HIP(hipStreamSynchronize(g_stream));     // a pass may still be running
    release(b);
    return Q4_OK;
}

int q4_batch_open(q4_batch* b, int slot, const int* prompt, int n_prompt, unsigned long long seed) {
    Q4_TRY(check_open(b, slot, prompt, n_prompt));
    return open_slot(b, slot, prompt, n_prompt, 0, seed);
}

int q4_batch_restore(q4_batch* b, int slot, const q4_snapshot* s, const int* prompt, int n_prompt, unsigned long long seed) {
    if (!s) return Q4_ERR_ARG;
    Q4_TRY(check_open(b, slot, prompt, n_prompt));
    const Model* m = model(b);
    const Config* p = &b->t->config;
    struct q4_snapshot_info i;
    Q4_TRY(q4_snapshot_info(s, &i));
    if (!m || i.fingerprint != m->fingerprint || i.kv_format != m->kv_format || i.n_layers != p->n_layers || i.n_kv_heads != p->n_kv_heads ||
        i.head_size != p->dim / p->n_heads || i.rope_theta != p->rope_theta || i.n_pos > p->seq_len || i.n_pos >= n_prompt)
        return Q4_ERR_ARG;
    if (memcmp(prompt, snapshot_token_ids(s), (size_t)i.n_pos * sizeof(int)) != 0) return Q4_ERR_ARG;
    // the packed K rows [layer][n_pos][kv_dim], then the V rows, into the slot's caches: one run per layer and cache
    const long long kv_dim = (long long)i.head_size * i.n_kv_heads, run = (long long)i.n_pos * kv_dim * (long long)sizeof(q4_half);
    const long long layer = (long long)p->seq_len * kv_dim * (long long)sizeof(q4_half);
    const char* packed = (const char*)snapshot_rows(s);
    const CopyRun runs[2] = {{b->k + (size_t)slot * b->cache_halves, packed, p->n_layers, layer, run, run},
                             {b->v + (size_t)slot * b->cache_halves, packed + (size_t)p->n_layers * run, p->n_layers, layer, run, run}};
    Q4_TRY(launch_copy_runs(runs, 2));
    return open_slot(b, slot, prompt, n_prompt, i.n_pos, seed);
}

int q4_batch_close(q4_batch* b, int slot) {
    if (!slot_ok(b, slot) || !b->open[slot]) return Q4_ERR_ARG;
    b->open[slot] = false;
    return Q4_OK;
}

int q4_batch_step(q4_batch* b, Sampler* sampler, int* tokens_out) {
    Model* m = model(b);
    if (!m || !sampler || !tokens_out || at_bound(b)) return Q4_ERR_ARG;
    Q4_TRY(step_admitted(b, m, sampler));
    Q4_TRY(queue_pass(b, m, sampler, b->words->out));
    Q4_HIP(hipMemcpyAsync(tokens_out, b->words->out, sizeof(int) * BATCH_MAX_SLOTS, hipMemcpyDeviceToHost, g_stream));
    Q4_HIP(hipStreamSynchronize(g_stream));
    return Q4_OK;
}

int q4_batch_generate(q4_batch* b, Sampler* sampler, int steps, int* out, int* n_out) {
    Model* m = model(b);
    if (!m || !sampler || !out || !n_out || steps < 1) return Q4_ERR_ARG;
    Q4_TRY(step_admitted(b, m, sampler));
    if (steps > b->log_passes) {
        Q4_HIP(hipStreamSynchronize(g_stream));
        if (b->log) (void)hipFree(b->log);
        b->log = nullptr;
        b->log_passes = 0;
        if (hipMalloc((void**)&b->log, (size_t)steps * BATCH_MAX_SLOTS * sizeof(int)) != hipSuccess) { (void)hipGetLastError(); b->log = nullptr; return Q4_ERR_ALLOC; }
        b->log_passes = steps;
    }
    int n = 0, rc = Q4_OK;
    while (n < steps && !at_bound(b) && !(rc = queue_pass(b, m, sampler, b->log + (size_t)n * BATCH_MAX_SLOTS))) n++;
    *n_out = n;                                              // (in front of the copy: the passes are queued whatever it returns)
    if (n) Q4_HIP(hipMemcpyAsync(out, b->log, (size_t)n * BATCH_MAX_SLOTS * sizeof(int), hipMemcpyDeviceToHost, g_stream));
    Q4_HIP(hipStreamSynchronize(g_stream));
    return rc;
}

int q4_batch_pos(const q4_batch* b, int slot) {
    if (!slot_ok(b, slot)) return -Q4_ERR_ARG;
    int pos = 0;
    if (hipStreamSynchronize(g_stream) != hipSuccess || hipMemcpy(&pos, &b->words->pos[slot], sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) return -Q4_ERR_HIP;
    return pos;
}

int q4_batch_get_logits(const q4_batch* b, int slot, q4_half* host_out) {
    if (!slot_ok(b, slot) || !host_out) return Q4_ERR_ARG;
    const size_t vocab = (size_t)b->t->config.vocab_size;
    Q4_HIP(hipStreamSynchronize(g_stream));
    Q4_HIP(hipMemcpy(host_out, b->logits + (size_t)slot * vocab, vocab * sizeof(q4_half), hipMemcpyDeviceToHost));
    return Q4_OK;
}

int q4_batch_get_kv_row(const q4_batch* b, int slot, int layer, int pos, q4_half* host_k, q4_half* host_v) {
    if (!slot_ok(b, slot) || !host_k || !host_v) return Q4_ERR_ARG;
    const Config* p = &b->t->config;
    if (layer < 0 || layer >= p->n_layers || pos < 0 || pos >= p->seq_len) return Q4_ERR_ARG;
    const size_t kv_dim = (size_t)p->dim / p->n_heads * p->n_kv_heads;
    const size_t off = (size_t)slot * b->cache_halves + ((size_t)layer * p->seq_len + pos) * kv_dim;
    Q4_HIP(hipStreamSynchronize(g_stream));
    Q4_HIP(hipMemcpy(host_k, b->k + off, kv_dim * sizeof(q4_half), hipMemcpyDeviceToHost));
    Q4_HIP(hipMemcpy(host_v, b->v + off, kv_dim * sizeof(q4_half), hipMemcpyDeviceToHost));
    return Q4_OK;
}

int q4_batch_cache(const q4_batch* b, int slot, q4_half** key_cache, q4_half** value_cache) {
    if (!slot_ok(b, slot) || !key_cache || !value_cache) return Q4_ERR_ARG;
    *key_cache = b->k + (size_t)slot * b->cache_halves;
    *value_cache = b->v + (size_t)slot * b->cache_halves;
    return Q4_OK;
}

}  // extern "C"
