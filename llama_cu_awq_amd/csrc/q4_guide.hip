// q4_guide.hip -- guided decoding: a token automaton masks the step's fp16 logits in place, in front of the sampling controls' launch and the argmax
// or the sampler. Not in the reference.
// A guide is a dense table next[S][V] of uint16_t (a state in [0, S), or Q4_GUIDE_DEAD: the state forbids the token), immutable, on the device as S rows of
// V rounded up to 8 entries -- a row is read in 16-byte pieces --: 2 * S * V bytes, 64 KB per state at 32000 tokens, 262 MB at the 4096 states a guide may
// have. The automaton's state lives on the device by position, in a ring state[seq_len] of int per model (Q4_GUIDE_NONE: no guided step ran here,
// Q4_GUIDE_OFFTRACK: a token the guide forbids was consumed; sticky).
// ONE 1024-thread block, the partition of logit_block.h: thread t owns the 16-byte chunks t, t + 1024, ... and, past the last
// whole chunk, one tail element. With p = *pPos:
//   1. prev = p > 0 ? state[p - 1] : NONE
//   2. s = 0 if prev == NONE; OFFTRACK if prev == OFFTRACK or prev is outside [0, S); else with t = tokens[p] (the pinned ring, read by position the way
//      copy_embedding_kernel and the penalty window read it): next[prev][t] if 0 <= t < V and the entry is a state, else OFFTRACK
//   3. state[p] = s (one lane, a plain store)
//   4. s != OFFTRACK: every i < n with next[s][i] == DEAD becomes the half 0xFC00 (-inf); every other entry keeps its 16 bits -- NaN payloads, -0 and
//      infinities included. s == OFFTRACK: the logits stay as they are.
// The thread's first four chunks of the logits (all of them up to 32 x 1024 logits) are requested BEFORE the dependent chain p -> state[p - 1] ->
// tokens[p] -> next[prev][t] -- four dependent reads (the position beside the block's fields, the state, the ring entry, the table's entry), one of
// them across PCIe -- so the chain hides behind the logits' load instead of standing in front of
// it; larger vocabularies read the rest in a loop behind the chain. No atomics, no arrival order: the same input gives the same bytes on every launch.
// Nothing that comes out of memory indexes anything unchecked: p against [0, seq_len), prev and the table's entry against [0, S), t against [0, V) -- a
// garbage ring gives OFFTRACK, never a read out of bounds.
// The row form (ROWS; a verify pass with q4_set_pass_stages on, q4_guide_mask_rows): block r of up to PROMPT_PASS_MAX is row r -- its logits `ld` halves
// behind row 0's, its position pos_rows[r] = p0 + r (pPos points at the rows' positions), and `tokens` is the pass's draft view (by absolute position:
// the ring up to p0, the drafts behind it), not the pinned ring. state[p0 + r - 1] is what the step at the position in front would have written, so the
// block walks the chain itself: from state[p0 - 1] rule 2 is applied over tokens[p0] .. tokens[p0 + r], r + 1 dependent table reads on the same scalar
// path, and waits for no other block. It stores state[p0 + r] (one writer per word; no block reads what another writes) and masks with it.
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "q4_device.h"
#include "q4_model.h"
#include "logit_block.h"
#include "prompt_pass.h"
using namespace q4;

// the handle of the C ABI: the device table and how many live models hold it
struct q4_guide {
    uint16_t* table;     // device, [S][stride]
    int S, V, stride;    // stride: V rounded up to 8
    mutable int attached;   // (a guide is handed around as const: immutable but for this count)
    int* forced;         // host, [S][2], built once by q4_guide_new: the one live token of a state and the state behind it, {-1, -1} where the state has two or more live tokens
};

namespace {

constexpr int GM_Q = 4;                                // register-resident 16-byte chunks per thread (the block and its partition: logit_block.h)

// what the kernel reads: one small device block per model (or the op-level launcher's), rewritten in stream order when the guide changes, so a captured
// graph holds the block's address and nothing of the guide
struct GuideBlock {
    const uint16_t* table;
    int* state;
    int S, V, stride, seq_len;
};

__device__ __forceinline__ u32x4 mask_chunk(const u32x4& q, const u32x4& r, bool& changed) {
    u32x4 o = q;
#pragma unroll
    for (int d = 0; d < 4; d++) {
        const unsigned lo = (r[d] & 0xFFFFu) == 0xFFFFu ? 0xFFFFu : 0u, hi = (r[d] >> 16) == 0xFFFFu ? 0xFFFF0000u : 0u;
        const unsigned dead = lo | hi;
        o[d] = (q[d] & ~dead) | (0xFC00FC00u & dead);
        changed = changed || o[d] != q[d];
    }
    return o;
}

// The block's pointers come out of memory, so the compiler knows no address space for them and would read through them with flat VECTOR loads -- which
// return in order behind the logits' loads and would put the whole chain behind them. Cast to the global address space, the chain's reads are uniform
// loads on the scalar unit's own counter (the table's entry as the aligned 32-bit word that holds it: the scalar unit has no 16-bit load).
#define GM_GLOBAL __attribute__((address_space(1)))

template <bool ROWS = false>
__global__ void __launch_bounds__(LB_T) guide_mask_kernel(q4_half* logits, int n, const GuideBlock* __restrict__ blk, const int* tokens, const int* pPos, int ld) {
    const int tid = threadIdx.x;
    if (ROWS) logits += (size_t)blockIdx.x * ld;
    const int n8 = n >> 3, tail = n8 * 8 + tid;
    u32x4* lv = reinterpret_cast<u32x4*>(logits);
    // the logits first: their requests are in flight while the chain below resolves
    u32x4 pq[GM_Q];
#pragma unroll
    for (int kq = 0; kq < GM_Q; kq++) {
        const int u = tid + kq * LB_T;
        pq[kq] = u < n8 ? lv[u] : (u32x4){0u, 0u, 0u, 0u};
    }

    // ---- steps 1 - 3 (block-uniform: every thread resolves the same chain)
    const int p0 = *pPos, p = ROWS ? p0 + (int)blockIdx.x : p0;   // (ROWS: pPos[r] = pPos[0] + r, PassScratch::pos)
    const GM_GLOBAL uint16_t* table = (const GM_GLOBAL uint16_t*)blk->table;
    int* state = blk->state;
    const int S = blk->S, V = blk->V, stride = blk->stride, seq_len = blk->seq_len;
    if (p0 < 0 || p >= seq_len || n > stride) return;
    int prev = p0 > 0 ? ((const GM_GLOBAL int*)state)[p0 - 1] : (int)Q4_GUIDE_NONE;
    int s = Q4_GUIDE_OFFTRACK;
    for (int q = p0;; q++) {                                   // (ROWS false: one turn, the step's)
        s = Q4_GUIDE_OFFTRACK;
        if (prev == Q4_GUIDE_NONE) s = 0;
        else if (prev >= 0 && prev < S) {
            const int t = ROWS ? ((const GM_GLOBAL int*)tokens)[q] : tokens[q];
            if (t >= 0 && t < V) {
                const size_t at = (size_t)prev * stride + t;
                const int e = (int)((((const GM_GLOBAL uint32_t*)table)[at >> 1] >> ((at & 1) * 16)) & 0xFFFFu);
                if (e < S) s = e;                              // (DEAD is above every state)
            }
        }
        if (!ROWS || q == p) break;
        prev = s;
    }
    if (tid == 0) state[p] = s;
    if (s == Q4_GUIDE_OFFTRACK) return;

    // ---- step 4
    const GM_GLOBAL uint16_t* row = table + (size_t)s * stride;
    const GM_GLOBAL u32x4* rv = (const GM_GLOBAL u32x4*)row;
    u32x4 rq[GM_Q];                                            // (requested together: one wait for the row, not one per chunk)
#pragma unroll
    for (int kq = 0; kq < GM_Q; kq++) {
        const int u = tid + kq * LB_T;
        rq[kq] = u < n8 ? rv[u] : (u32x4){0u, 0u, 0u, 0u};
    }
#pragma unroll
    for (int kq = 0; kq < GM_Q; kq++) {
        const int u = tid + kq * LB_T;
        if (u < n8) {
            bool changed = false;
            const u32x4 o = mask_chunk(pq[kq], rq[kq], changed);
            if (changed) lv[u] = o;
        }
    }
    for (int u = tid + GM_Q * LB_T; u < n8; u += LB_T) {     // more than 32 x 1024 logits: the rest, chunk by chunk
        bool changed = false;
        const u32x4 q = lv[u], r = rv[u];
        const u32x4 o = mask_chunk(q, r, changed);
        if (changed) lv[u] = o;
    }
    if (tail < n && row[tail] == 0xFFFFu) logits[tail] = (q4_half)0xFC00u;
}

GuideBlock* g_op_block = nullptr;      // q4_guide_mask's own block

int launch(q4_half* logits, int n, const GuideBlock* dev, const int* tokens, const int* pPos) {
    Q4_LAUNCH(guide_mask_kernel<false>, dim3(1), dim3(LB_T), 0, logits, n, dev, tokens, pPos, 0);
    Q4_LAUNCH_CHECK();
    return Q4_OK;
}
// the row form: view the draft view (device), pos_rows the rows' positions (device)
int launch_rows_of(q4_half* logits, int n, int ld, int n_rows, const GuideBlock* dev, const int* view, const int* pos_rows) {
    if (n_rows < 1 || n_rows > PROMPT_PASS_MAX || ld < n || (ld & 7)) return Q4_ERR_ARG;
    Q4_LAUNCH(guide_mask_kernel<true>, dim3(n_rows), dim3(LB_T), 0, logits, n, dev, view, pos_rows, ld);
    Q4_LAUNCH_CHECK();
    return Q4_OK;
}

int ring_to_none(const Model* m, int first, int count) {
    if (first < 0 || count < 0 || first + count > m->guide_len) return Q4_ERR_ARG;
    Q4_HIP(hipMemsetAsync(m->guide_state + first, 0xFF, (size_t)count * sizeof(int), g_stream));
    return Q4_OK;
}

}  // namespace

namespace q4 {

// the stage lives with the model: q4_set_guide has allocated and written the block, nothing to prepare and nothing a Sampler owns
static bool stage_on(const Sampler*, const Model* m) { return m && m->guide; }
static int prepare(const Sampler*, Model* m, const Config*, const void** block) {
    *block = m->guide_block;
    return Q4_OK;
}
static int launch_step(const void* block, const Model*, const Config* p, RunState* s) {
    return launch(s->logits, p->vocab_size, (const GuideBlock*)block, &(s->shared_data->tokens[0]), s->pos);
}
static int launch_rows(const void* block, const Model*, const Config* p, q4_half* rows, int ld, int n_rows, const int* view, const int* pos_rows) {
    return launch_rows_of(rows, p->vocab_size, ld, n_rows, (const GuideBlock*)block, view, pos_rows);
}
LogitStage guide_stage = {stage_on, prepare, launch_step, nullptr, nullptr, launch_rows};
int guide_clear_positions(const Model* m, int pos, int nsteps) { return ring_to_none(m, pos, nsteps); }
int guide_clear_ring(const Model* m) { return ring_to_none(m, 0, m->guide_len); }
int guide_forced_draft(const Model* m, const int* ring, int pos, int max_draft, int* draft, int* n_out) {
    *n_out = 0;
    const q4_guide* g = m->guide;
    if (!g || !m->guide_state || pos < 0 || pos >= m->guide_len) return Q4_OK;
    int prev = Q4_GUIDE_NONE, s = Q4_GUIDE_OFFTRACK;
    if (pos > 0) Q4_HIP(hipMemcpy(&prev, m->guide_state + pos - 1, sizeof(int), hipMemcpyDeviceToHost));
    if (prev == Q4_GUIDE_NONE) s = 0;
    else if (prev >= 0 && prev < g->S) {
        const int t = ring[pos];
        if (t >= 0 && t < g->V) {
            uint16_t e = Q4_GUIDE_DEAD;
            Q4_HIP(hipMemcpy(&e, g->table + (size_t)prev * g->stride + t, sizeof(e), hipMemcpyDeviceToHost));
            if (e < g->S) s = e;
        }
    }
    *n_out = q4_guide_forced_run(g, s, max_draft, draft);
    return Q4_OK;
}
// q4_free_transformer: the graphs that hold the block are gone and the device has drained
void guide_release(Model* m) {
    if (m->guide) m->guide->attached--;
    if (m->guide_state) (void)hipFree(m->guide_state);
    if (m->guide_block) (void)hipFree(m->guide_block);
    m->guide = nullptr; m->guide_state = nullptr; m->guide_block = nullptr; m->guide_len = 0;
}

}  // namespace q4

extern "C" {

int q4_guide_new(q4_guide** out, int n_states, int vocab_size, const uint16_t* next) {
    if (!out || !next || n_states < 1 || n_states > Q4_GUIDE_MAX_STATES || vocab_size < 1) return Q4_ERR_ARG;
    for (int s = 0; s < n_states; s++) {
        const uint16_t* row = next + (size_t)s * vocab_size;
        bool live = false;
        for (int i = 0; i < vocab_size; i++) {
            if (row[i] == Q4_GUIDE_DEAD) continue;
            if (row[i] >= n_states) return Q4_ERR_ARG;
            live = true;
        }
        if (!live) return Q4_ERR_ARG;
    }
    const int stride = (vocab_size + 7) / 8 * 8;
    const size_t bytes = (size_t)n_states * stride * sizeof(uint16_t);
    uint16_t* table = nullptr;
    if (hipMalloc((void**)&table, bytes) != hipSuccess) { (void)hipGetLastError(); return Q4_ERR_ALLOC; }
    std::vector<uint16_t> padded((size_t)n_states * stride, (uint16_t)Q4_GUIDE_DEAD);
    for (int s = 0; s < n_states; s++) memcpy(&padded[(size_t)s * stride], next + (size_t)s * vocab_size, (size_t)vocab_size * sizeof(uint16_t));
    if (hipMemcpy(table, padded.data(), bytes, hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipGetLastError();
        (void)hipFree(table);
        return Q4_ERR_HIP;
    }
    q4_guide* g = (q4_guide*)calloc(1, sizeof(q4_guide));
    int* forced = (int*)malloc((size_t)n_states * 2 * sizeof(int));
    if (!g || !forced) { (void)hipFree(table); free(g); free(forced); return Q4_ERR_ALLOC; }
    for (int s = 0; s < n_states; s++) {                       // (every state has a live token: checked above)
        const uint16_t* row = next + (size_t)s * vocab_size;
        int tok = -1, live = 0;
        for (int i = 0; i < vocab_size && live < 2; i++)
            if (row[i] != Q4_GUIDE_DEAD) { tok = i; live++; }
        forced[2 * s] = live == 1 ? tok : -1;
        forced[2 * s + 1] = live == 1 ? (int)row[tok] : -1;
    }
    g->table = table; g->S = n_states; g->V = vocab_size; g->stride = stride; g->forced = forced;
    *out = g;
    return Q4_OK;
}
int q4_guide_delete(q4_guide* g) {
    if (!g || g->attached > 0) return Q4_ERR_ARG;
    if (g_stream) Q4_HIP(hipStreamSynchronize(g_stream));     // a launch of a model that held it until a moment ago may still read the table
    Q4_HIP(hipFree(g->table));
    free(g->forced);
    free(g);
    return Q4_OK;
}

// The forced tokens from `state`: while the state has exactly one live token, that token, and on to the state behind it. At most max_draft; the run ends
// behind an EOS (token 2). 0 for a state outside [0, S) (Q4_GUIDE_NONE and Q4_GUIDE_OFFTRACK are), a null argument or max_draft < 1.
int q4_guide_forced_run(const q4_guide* g, int state, int max_draft, int* draft_out) {
    if (!g || !draft_out || max_draft < 1) return 0;
    int n = 0;
    while (n < max_draft && state >= 0 && state < g->S && g->forced[2 * state] >= 0) {
        const int tok = g->forced[2 * state];
        draft_out[n++] = tok;
        if (tok == 2) break;
        state = g->forced[2 * state + 1];
    }
    return n;
}

int q4_set_guide(Transformer* t, const q4_guide* g) {
    Model* m = t ? model_of(&t->state) : nullptr;
    if (!m || (g && g->V != t->config.vocab_size)) return Q4_ERR_ARG;
    if (!g && !m->guide) return Q4_OK;                         // off, and (possibly) never on: nothing to allocate or clear
    if (g && !m->guide_block) {                                // the first guide of this model: the ring and the block, kept until q4_free_transformer
        int* ring = nullptr;
        void* block = nullptr;
        if (hipMalloc((void**)&ring, (size_t)t->config.seq_len * sizeof(int)) != hipSuccess || hipMalloc(&block, sizeof(GuideBlock)) != hipSuccess) {
            (void)hipGetLastError();
            if (ring) (void)hipFree(ring);
            return Q4_ERR_ALLOC;
        }
        m->guide_state = ring;
        m->guide_len = t->config.seq_len;
        m->guide_block = block;
    }
    if (g && g != m->guide) {                                  // (pageable: staged before the call returns)
        const GuideBlock host = {g->table, m->guide_state, g->S, g->V, g->stride, m->guide_len};
        Q4_HIP(hipMemcpyAsync(m->guide_block, &host, sizeof(host), hipMemcpyHostToDevice, g_stream));
    }
    if (m->guide) m->guide->attached--;
    if (g) g->attached++;
    m->guide = g;
    return guide_clear_ring(m);
}
const q4_guide* q4_get_guide(const Transformer* t) {
    const Model* m = t ? model_of(&t->state) : nullptr;
    return m ? m->guide : nullptr;
}
int q4_get_guide_states(const Transformer* t, int first_pos, int n, int* out) {
    const Model* m = t ? model_of(&t->state) : nullptr;
    if (!m || !m->guide || !out || first_pos < 0 || n < 0 || (long long)first_pos + n > m->guide_len) return Q4_ERR_ARG;
    Q4_HIP(hipStreamSynchronize(g_stream));
    if (n > 0) Q4_HIP(hipMemcpy(out, m->guide_state + first_pos, (size_t)n * sizeof(int), hipMemcpyDeviceToHost));
    return Q4_OK;
}

int q4_guide_mask(q4_half* logits, int n, const q4_guide* g, int* state_ring, const int* tokens, const int* pPos) {
    if (!logits || !g || n != g->V || !state_ring || !tokens || !pPos) return Q4_ERR_ARG;
    if (!g_op_block) Q4_HIP(hipMalloc((void**)&g_op_block, sizeof(GuideBlock)));
    const GuideBlock host = {g->table, state_ring, g->S, g->V, g->stride, Q4_MAX_SEQ_LEN};
    Q4_HIP(hipMemcpyAsync(g_op_block, &host, sizeof(host), hipMemcpyHostToDevice, g_stream));   // (pageable: staged before the call returns)
    return launch(logits, n, g_op_block, tokens, pPos);
}
int q4_guide_mask_rows(q4_half* logits, int n, const q4_guide* g, int* state_ring, int ld, int n_rows, const int* tokens_view_dev, const int* pos_rows_dev) {
    if (!logits || !g || n != g->V || !state_ring || !tokens_view_dev || !pos_rows_dev || n_rows < 1 || n_rows > PROMPT_PASS_MAX || ld < n || (ld & 7)) return Q4_ERR_ARG;
    if (!g_op_block) Q4_HIP(hipMalloc((void**)&g_op_block, sizeof(GuideBlock)));
    const GuideBlock host = {g->table, state_ring, g->S, g->V, g->stride, Q4_MAX_SEQ_LEN};
    Q4_HIP(hipMemcpyAsync(g_op_block, &host, sizeof(host), hipMemcpyHostToDevice, g_stream));   // (pageable: staged before the call returns)
    return launch_rows_of(logits, n, ld, n_rows, g_op_block, tokens_view_dev, pos_rows_dev);
}

}  // extern "C"
