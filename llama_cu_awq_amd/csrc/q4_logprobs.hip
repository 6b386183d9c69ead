// q4_logprobs.hip -- per-token log-probabilities and top-k alternatives of the model's OWN distribution (temperature 1, no nucleus: not
// what the sampler drew from), computed from the step's fp16 logits before the sampler destroys them, and the record ring's switch and read-out. Not in the reference.
//   lse = m + logf(sum_i expf(l_i - m)), m = max_i l_i, fp32; a log-probability is l - lse (one fp32 subtraction).
// ONE 1024-thread block (the argmax launch beside it is one block too; the whole vocabulary is 64 KB of L2 hits):
//   * thread t owns the 16-byte chunks t, t + 1024, ... (8 consecutive logits each) and, past the last whole chunk, one tail element -- argmax_kernel's
//     partition (logit_block.h: the other single-block launches over the logits use it too). Up to 32 x 1024 logits stay in registers between the phases; larger vocabularies re-read them from L2 in every phase.
//   * the sum has a fixed order: a thread adds runs of 32 exponentials (four chunks) in ascending index, adds the runs' totals in ascending order
//     (one run up to 32 x 1024 logits, four at 128256), then the tail element; a 64-lane tree (wave_sum), a 16-lane tree over the wave totals.
//     No atomics, no arrival order, never more than 32 + runs + 1 sequential adds: bit-stable from launch to launch.
//   * top-k is exact on the 16-bit monotone key of the half (-0 counts as +0, NaN ranks last; ties: ascending index -- argmax_kernel's rule, so entry 0
//     is the greedy token). Every element has a unique 64-bit word P = (key + 1) << 32 | ~index; larger P = earlier in the order. The k-th largest of
//     the 1024 THREAD maxima, T, is found without block-wide reductions (each wave extracts the k largest of its 64 maxima by k butterflies, wave 0
//     the k largest of those 16 x k); at least k elements are >= T, and the elements >= T live in exactly k threads, so at most k x (elements per
//     thread) of them exist -- usually k plus a few. They are appended to an LDS list in any order (an integer counter) and each finds its rank by
//     counting the larger ones: rank r < k writes entry r.
// The row form (ROWS; prompt and verify passes with q4_set_pass_logprobs on, q4_logprob_topk_rows): block r of up to PROMPT_PASS_MAX is row r -- its logits
// `ld` halves behind row 0's, its record *pPos + r, its side copy side + r * n -- and everything between is the step's, one body: a row's record is, byte
// for byte, what the one-block launch writes for that row alone. The halves between n and ld are neither read nor written.
#include <hip/hip_runtime.h>
#include <math.h>
#include "q4_device.h"
#include "q4_model.h"
#include "logit_block.h"
#include "prompt_pass.h"
using namespace q4;

namespace {

constexpr int LP_Q = 4;                                // register-resident 16-byte chunks per thread
constexpr int LP_K = Q4_MAX_TOP_LOGPROBS;
// LDS candidate list: k x (elements per thread) entries always fit. In registers a thread has 32 + 1 elements: 20 x 33 = 660; the looping path's list
// fills what is left of 64 KB of static LDS (k x (8 x chunks per thread + 1) <= 6144: 311,000 logits at k = 20; the launcher refuses more)
constexpr int LP_CAND_REG = LP_K * (LP_Q * 8 + 1), LP_CAND_LOOP = 6144;

typedef unsigned long long u64;

// (half_key, the monotone key of a half, and half_of: logit_block.h)
__device__ __forceinline__ u64 pack_p(unsigned key, unsigned idx) { return ((u64)(key + 1u) << 32) | (u64)(0xFFFFFFFFu - idx); }
__device__ __forceinline__ unsigned p_index(u64 p) { return 0xFFFFFFFFu - (unsigned)p; }

__device__ __forceinline__ u64 wave_max_u64(u64 v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)v, off), hi = (unsigned)__shfl_xor((int)(unsigned)(v >> 32), off);
        const u64 o = ((u64)hi << 32) | lo;
        v = o > v ? o : v;
    }
    return v;
}

// REG: n <= 32 x 1024, the thread's chunks stay in registers. mode: LP_TARGET the target token is tokens[tok_off + position] (tokens null: none),
// LP_GREEDY token_logprob = entry 0, LP_SAMPLED the raw logits go to `side` and logprob_pick_kernel fills token_logprob behind the sampler.
// pPos null: the stand-alone launcher (record 0); else record *pPos of rings with `cap` records -- a position outside them writes nothing.
// ROWS: the row form of the header -- block r reads logits + r * ld and stands at position (*pPos, or 0) + r; nothing else differs.
template <bool REG, bool ROWS = false>
__global__ void __launch_bounds__(LB_T) logprob_topk_kernel(const q4_half* __restrict__ logits, int n, int top_k, int mode, const int* tokens, int tok_off,
                                                            const int* pPos, int cap, float* lse_out, float* tlp_out, int* top_ids, float* top_lps,
                                                            q4_half* __restrict__ side, int ld) {
    constexpr int LP_CAND = REG ? LP_CAND_REG : LP_CAND_LOOP;
    __shared__ u64 cand[LP_CAND];
    __shared__ u64 wtop[LB_W * LP_K];
    __shared__ float red[16];
    __shared__ u64 s_T;
    __shared__ unsigned s_count;
    __shared__ int s_top0;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int pos = (pPos ? *pPos : 0) + (ROWS ? (int)blockIdx.x : 0);
    if (pPos && (pos < 0 || pos >= cap)) return;               // (block-uniform)
    if (ROWS) {
        logits += (size_t)blockIdx.x * ld;
        if (side != nullptr) side += (size_t)blockIdx.x * n;
    }
    // the target token may sit in pinned host memory (the token ring): requested first, used last
    int target = -1;
    if (mode == LP_TARGET && tokens != nullptr && tid == 0 && tok_off + pos < Q4_MAX_SEQ_LEN) target = tokens[tok_off + pos];
    const int keff = top_k > 0 ? top_k : 1;                    // entry 0 is always found: the greedy token
    const int n8 = n >> 3, nq = REG ? LP_Q : (n8 + LB_T - 1) / LB_T;
    const int tail = n8 * 8 + tid;                             // this thread's tail element, if < n
    const u32x4* lv = reinterpret_cast<const u32x4*>(logits);
    u32x4 pq[LP_Q];
    if (REG) {
#pragma unroll
        for (int kq = 0; kq < LP_Q; kq++) {
            const int u = tid + kq * LB_T;
            pq[kq] = u < n8 ? lv[u] : (u32x4){0u, 0u, 0u, 0u};
        }
    }
    const unsigned th = tail < n ? (unsigned)logits[tail] : 0u;
    if (tid == 0) { s_count = 0u; s_top0 = 0; }

    // ---- phase 1: thread maximum (float, for the sum) and the thread's best element in the order (first of equal keys: ascending scan)
    float m = -INFINITY;
    int best_key = -1;
    unsigned best_idx = 0;
#pragma unroll 4
    for (int kq = 0; kq < (REG ? LP_Q : nq); kq++) {
        const int u = tid + kq * LB_T;
        if (u < n8) {
            u32x4 q;
            if constexpr (REG) q = pq[kq]; else q = lv[u];
#pragma unroll
            for (int e = 0; e < 8; e++) {
                const unsigned h = half_of(q, e);
                m = fmaxf(m, h2f((uint16_t)h));
                const int key = (int)half_key(h);
                if (key > best_key) { best_key = key; best_idx = (unsigned)u * 8u + e; }
            }
        }
    }
    if (tail < n) {
        m = fmaxf(m, h2f((uint16_t)th));
        const int key = (int)half_key(th);
        if (key > best_key) { best_key = key; best_idx = (unsigned)tail; }
    }
    const u64 mineP = best_key >= 0 ? pack_p((unsigned)best_key, best_idx) : 0ull;      // 0: a thread without elements
    // the wave's keff largest thread maxima: lane i keeps the i-th
    {
        u64 left = mineP, keep = 0ull;
        for (int i = 0; i < keff; i++) {
            const u64 w = wave_max_u64(left);
            if (lane == i) keep = w;
            if (left == w) left = 0ull;                        // (the words are unique; 0 stays 0)
        }
        if (lane < keff) wtop[wave * LP_K + lane] = keep;
    }
    m = wave_max(m);
    if (lane == 0) red[wave] = m;
    __syncthreads();
    m = row16_max(red[lane & 15]);
    // wave 0: T = the keff-th largest of the 16 x keff (0 when fewer than keff threads hold elements: every element is a candidate then)
    if (wave == 0) {
        u64 v[(LB_W * LP_K + 63) / 64];
#pragma unroll
        for (int j = 0; j < (LB_W * LP_K + 63) / 64; j++) {
            const int i = lane + 64 * j, w = i / LP_K, r = i - w * LP_K;
            v[j] = (i < LB_W * LP_K && r < keff) ? wtop[i] : 0ull;
        }
        u64 T = 0ull;
        for (int i = 0; i < keff; i++) {
            u64 l = v[0];
#pragma unroll
            for (int j = 1; j < (LB_W * LP_K + 63) / 64; j++) l = v[j] > l ? v[j] : l;
            T = wave_max_u64(l);
#pragma unroll
            for (int j = 0; j < (LB_W * LP_K + 63) / 64; j++) if (v[j] == T) v[j] = 0ull;
        }
        if (lane == 0) s_T = T;
    }

    // ---- phase 2: the sum of exponentials in the fixed order of the header
    float total = 0.f;
    {
        float run = 0.f;
#pragma unroll 4
        for (int kq = 0; kq < (REG ? LP_Q : nq); kq++) {
            const int u = tid + kq * LB_T;
            if (u < n8) {
                u32x4 q;
                if constexpr (REG) q = pq[kq]; else q = lv[u];
#pragma unroll
                for (int e = 0; e < 8; e++) run += expf(h2f((uint16_t)half_of(q, e)) - m);
            }
            if ((kq & (LP_Q - 1)) == LP_Q - 1) { total += run; run = 0.f; }      // a run of 32 is complete
        }
        if (!REG && (nq & (LP_Q - 1))) total += run;                               // the last, shorter run
        if (tail < n) total += expf(h2f((uint16_t)th) - m);
    }
    total = wave_sum(total);
    __syncthreads();                                           // (red is read by every thread above; s_T and s_count are written)
    if (lane == 0) red[wave] = total;
    __syncthreads();
    const float sum = row16_sum(red[lane & 15]);
    const float lse = m + logf(sum);

    // ---- phase 3: the elements >= T (only threads whose own maximum reaches it hold any)
    const u64 T = s_T;
    if (mineP >= T) {
#pragma unroll 4
        for (int kq = 0; kq < (REG ? LP_Q : nq); kq++) {
            const int u = tid + kq * LB_T;
            if (u < n8) {
                u32x4 q;
                if constexpr (REG) q = pq[kq]; else q = lv[u];
#pragma unroll
                for (int e = 0; e < 8; e++) {
                    const u64 p = pack_p(half_key(half_of(q, e)), (unsigned)u * 8u + e);
                    if (p >= T) {
                        const unsigned slot = atomicAdd(&s_count, 1u);
                        if (slot < (unsigned)LP_CAND) cand[slot] = p;
                    }
                }
            }
        }
        if (tail < n) {
            const u64 p = pack_p(half_key(th), (unsigned)tail);
            if (p >= T) {
                const unsigned slot = atomicAdd(&s_count, 1u);
                if (slot < (unsigned)LP_CAND) cand[slot] = p;
            }
        }
    }
    if (mode == LP_SAMPLED && side != nullptr) {               // the sampler overwrites `logits`: keep the raw values for logprob_pick_kernel
        for (int u = tid; u < n8; u += LB_T) reinterpret_cast<u32x4*>(side)[u] = lv[u];
        if (tail < n) side[tail] = (q4_half)th;
    }
    __syncthreads();
    const int count = (int)min(s_count, (unsigned)LP_CAND);
    const size_t rec = (size_t)pos;
    for (int i = tid; i < count; i += LB_T) {
        const u64 mine = cand[i];
        int r = 0;
        for (int j = 0; j < count; j++) r += cand[j] > mine ? 1 : 0;             // (every lane reads one word: an LDS broadcast)
        if (r < keff) {
            const unsigned idx = p_index(mine);
            if (idx < (unsigned)n) {                                               // (always: the words come from real elements)
                if (r < top_k) {
                    top_ids[rec * top_k + r] = (int)idx;
                    top_lps[rec * top_k + r] = h2f(logits[idx]) - lse;
                }
                if (r == 0) s_top0 = (int)idx;
            }
        }
    }
    if (mode == LP_GREEDY) __syncthreads();                    // (uniform: a kernel argument)
    if (tid == 0) {
        lse_out[rec] = lse;
        float tlp = __builtin_nanf("");                        // no (valid) target
        if (mode == LP_GREEDY) tlp = h2f(logits[s_top0]) - lse;
        else if (mode == LP_TARGET && target >= 0 && target < n) tlp = h2f(logits[target]) - lse;
        tlp_out[rec] = tlp;                                    // (sampled steps: NaN until logprob_pick_kernel has run behind the sampler)
    }
}

// behind the sampler launch of a sampled step: the position has advanced, the chosen token is tokens[position]; its raw logit comes from the side copy
// ROWS (a verify pass under the sampler, behind the row form of the sampler and in front of the accept launch: the position has NOT advanced): block r is
// row r -- record *pPos + r, the token tokens[r] (what the sampler's row form left), the side copy side + r * n.
template <bool ROWS>
__global__ void __launch_bounds__(64) logprob_pick_kernel(const q4_half* __restrict__ side, int n, const int* tokens, const int* pPos, int cap,
                                                          const float* lse_ring, float* tlp_ring) {
    if (threadIdx.x != 0) return;
    const int pos = *pPos, rec = ROWS ? pos + (int)blockIdx.x : pos - 1;
    if (rec < 0 || rec >= cap || (!ROWS && pos >= Q4_MAX_SEQ_LEN)) return;
    const int tok = ROWS ? tokens[blockIdx.x] : tokens[pos];
    if (ROWS) side += (size_t)blockIdx.x * n;
    tlp_ring[rec] = (tok >= 0 && tok < n) ? h2f(side[tok]) - lse_ring[rec] : __builtin_nanf("");
}

// n_rows 0: the step's one-block launch. Else the row form: n_rows blocks (1 .. PROMPT_PASS_MAX), rows `ld` halves apart (a multiple of 8: the rows stay
// 16-byte aligned; >= n)
int launch_topk(const q4_half* logits, int n, int top_k, int mode, const int* tokens, int tok_off, const int* pPos, int cap, float* lse, float* tlp,
                int* top_ids, float* top_lps, q4_half* side, int ld = 0, int n_rows = 0) {
    if (n < 1 || top_k < 0 || top_k > LP_K || top_k > n) return Q4_ERR_ARG;
    if (n_rows && (n_rows < 1 || n_rows > PROMPT_PASS_MAX || ld < n || (ld & 7))) return Q4_ERR_ARG;
    if (!logprobs_size_ok(n, top_k)) return Q4_ERR_UNSUPPORTED_SIZE;
    const bool reg = n <= LB_T * LP_Q * 8;
    if (n_rows && reg)
        Q4_LAUNCH((logprob_topk_kernel<true, true>), dim3(n_rows), dim3(LB_T), 0, logits, n, top_k, mode, tokens, tok_off, pPos, cap, lse, tlp, top_ids, top_lps, side, ld);
    else if (n_rows)
        Q4_LAUNCH((logprob_topk_kernel<false, true>), dim3(n_rows), dim3(LB_T), 0, logits, n, top_k, mode, tokens, tok_off, pPos, cap, lse, tlp, top_ids, top_lps, side, ld);
    else if (reg)
        Q4_LAUNCH(logprob_topk_kernel<true>, dim3(1), dim3(LB_T), 0, logits, n, top_k, mode, tokens, tok_off, pPos, cap, lse, tlp, top_ids, top_lps, side, ld);
    else
        Q4_LAUNCH(logprob_topk_kernel<false>, dim3(1), dim3(LB_T), 0, logits, n, top_k, mode, tokens, tok_off, pPos, cap, lse, tlp, top_ids, top_lps, side, ld);
    Q4_LAUNCH_CHECK();
    return Q4_OK;
}

}  // namespace

namespace q4 {

// the candidate list holds the elements of k threads: k x (8 per chunk + the tail element)
bool logprobs_size_ok(int n, int top_k) {
    const long long per_thread = 8ll * (((n >> 3) + LB_T - 1) / LB_T) + 1;
    return n <= LB_T * LP_Q * 8 || (long long)(top_k > 0 ? top_k : 1) * per_thread <= LP_CAND_LOOP;
}

int launch_logprobs_step(const Model* m, const Config* p, RunState* s, int gen_token, bool greedy) {
    const int mode = !gen_token ? LP_TARGET : greedy ? LP_GREEDY : LP_SAMPLED;
    // a prompt step's target is the NEXT ring entry, tokens[position + 1] (read the way copy_embedding_kernel reads its own)
    return launch_topk(s->logits, p->vocab_size, m->logprobs_k, mode, &(s->shared_data->tokens[0]), 1, s->pos, p->seq_len, m->lp_lse, m->lp_token,
                       m->lp_ids, m->lp_top, m->lp_side);
}
int launch_logprobs_pick(const Model* m, const Config* p, RunState* s) {
    Q4_LAUNCH(logprob_pick_kernel<false>, dim3(1), dim3(64), 0, m->lp_side, p->vocab_size, &(s->shared_data->tokens[0]), s->pos, p->seq_len, m->lp_lse, m->lp_token);
    Q4_LAUNCH_CHECK();
    return Q4_OK;
}
// The records of a pass (prompt_pass.h, spec_verify.h): row r < n of `rows` (ld halves apart) holds the logits at position *s->pos + r, and record
// *s->pos + r of the model's rings is what the step at that position writes. LP_TARGET: the target of row r is the ring's tokens[*s->pos + r + 1] (prompt
// passes, scoring); LP_GREEDY: entry 0 (greedy verify passes); LP_SAMPLED: the raw rows go to the pass's side rows (Model::pass.lp_side) and
// launch_logprobs_pick_rows fills token_logprob behind the row form of the sampler. In front of the launch that advances the position.
int launch_logprobs_rows(const Model* m, const Config* p, RunState* s, const q4_half* rows, int ld, int n, int mode) {
    if (!m || m->logprobs_k < 0 || !rows || (mode == LP_SAMPLED && !m->pass.lp_side)) return Q4_ERR_ARG;
    return launch_topk(rows, p->vocab_size, m->logprobs_k, mode, &(s->shared_data->tokens[0]), 1, s->pos, p->seq_len, m->lp_lse, m->lp_token, m->lp_ids,
                       m->lp_top, mode == LP_SAMPLED ? m->pass.lp_side : nullptr, ld, n);
}
int launch_logprobs_pick_rows(const Model* m, const Config* p, RunState* s, int n, const int* win) {
    if (!m || m->logprobs_k < 0 || !m->pass.lp_side || !win || n < 1 || n > PROMPT_PASS_MAX) return Q4_ERR_ARG;
    Q4_LAUNCH(logprob_pick_kernel<true>, dim3(n), dim3(64), 0, m->pass.lp_side, p->vocab_size, win, s->pos, p->seq_len, m->lp_lse, m->lp_token);
    Q4_LAUNCH_CHECK();
    return Q4_OK;
}

}  // namespace q4

extern "C" int q4_logprob_topk(const q4_half* logits, int n, int top_k, const int* target, float* lse, float* target_logprob, int* top_ids,
                               float* top_logprobs) {
    if (!logits || !lse || !target_logprob || (top_k > 0 && (!top_ids || !top_logprobs))) return Q4_ERR_ARG;
    return launch_topk(logits, n, top_k, LP_TARGET, target, 0, nullptr, 1, lse, target_logprob, top_ids, top_logprobs, nullptr);
}
// The row form on rows the caller holds (include/llama2_q4.h): for tests and tools. Row r is "position" r: its target targets[r], its outputs entry r
extern "C" int q4_logprob_topk_rows(const q4_half* logits, int ld, int n, int n_rows, int top_k, const int* targets, float* lse, float* target_logprob,
                                    int* top_ids, float* top_logprobs) {
    if (!logits || !lse || !target_logprob || (top_k > 0 && (!top_ids || !top_logprobs))) return Q4_ERR_ARG;
    if (n_rows < 1 || n_rows > PROMPT_PASS_MAX || ld < n || (ld & 7)) return Q4_ERR_ARG;
    return launch_topk(logits, n, top_k, LP_TARGET, targets, 0, nullptr, 1, lse, target_logprob, top_ids, top_logprobs, nullptr, ld, n_rows);
}

// the record ring: the per-model switch and the read-out (teacher-forced scoring over them: q4_loops.hip's q4_score_ids)
extern "C" int q4_set_logprobs(Transformer* t, int top_k) {
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
extern "C" int q4_get_logprobs_k(const Transformer* t) {
    const Model* m = t ? model_of(&t->state) : nullptr;
    return m ? m->logprobs_k : -1;
}
extern "C" int q4_get_logprobs(const Transformer* t, int first_pos, int n, float* token_logprob, int* top_ids, float* top_logprobs) {
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
