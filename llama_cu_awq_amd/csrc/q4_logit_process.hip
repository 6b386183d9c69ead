// q4_logit_process.hip -- the sampling controls of a completion API beside temperature and top-p: logit bias, repetition / presence / frequency penalties,
// top-k and min-p, as ONE launch that rewrites the step's fp16 logits in place in front of the argmax or the sampler. Not in the reference.
// ONE 1024-thread block, the partition of logit_block.h: thread t owns the 16-byte chunks t, t + 1024, ... and, past the last whole chunk, one tail
// element; up to 32 x 1024 logits stay in registers, larger vocabularies are read again from L2 in every pass.
//   1. bias, 2. penalties, 3. clamp and round -- on the TOUCHED entries only (at most 256 bias ids and 1024 window tokens):
//      v = float(l); v += b_i; with c_i > 0 occurrences of i in the window: v = v > 0 ? v / r : v * r, v -= (float(c_i) * frequency + presence);
//      a finite v is clamped to +-65504 and rounded to half (RNE), an infinity stays, a NaN result is the quiet NaN 0x7E00. Every operation is one IEEE
//      fp32 operation (no contraction: numpy float32 reproduces the bits).
//      The window is the ring entries tokens[max(0, pos + 1 - last_n) .. pos], pos = *pPos before the sampler advances it: prompt tokens count, entries
//      outside [0, n) do not. It is read from the ring by position in every launch -- no state, nothing to reset or rewind -- and only when a penalty is
//      not neutral. The ring is pinned host memory: thread t requests entry t first; the bias list is staged while the request is in flight. The
//      occurrences are counted in LDS: every thread compares its entry with all the others (last_n / 4 broadcast reads of 16 bytes), the first occurrence
//      of a token rewrites its logit, a bias id that is also in the window hands its bias to that thread through LDS.
//   4. top-k on the 16-bit monotone key of a half (logit_block.h; -0 equals +0, NaN ranks last), order (key descending, index ascending): T, the k-th largest
//      key, by 16 steps of a binary search whose count is one block-wide sum each; with ties that straddle rank k the entries equal to T keep their place
//      by index (one block-wide prefix sum per row of 8192 logits, until the k are full). Everything behind rank k becomes -inf.
//   5. min-p on the PROCESSED logits at temperature 1 (independent of the sampler's temperature): with m the largest of them, entry i stays iff
//      float(l_i) - float(m) >= logf(min_p) (the host's logf, a kernel argument); else -inf.
// No atomics, no arrival order: the same input gives the same bytes on every launch. A NaN or an out-of-range token never faults: the window and the
// bias ids are checked against [0, n) before they index anything.
// The row form (ROWS; a verify pass with q4_set_pass_stages on, q4_process_logits_rows): block r of up to PROMPT_PASS_MAX is row r -- its logits `ld` halves
// behind row 0's, its position pPos[r], and `tokens` is the pass's draft view (by absolute position: the ring up to the pass's first position, the drafts
// behind it), not the pinned ring. Everything between those three substitutions is the step's one body.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include <map>
#include "q4_device.h"
#include "q4_model.h"
#include "sampler_side.h"
#include "logit_block.h"
#include "option_text.h"
#include "prompt_pass.h"
#pragma clang fp contract(off)
using namespace q4;

namespace {

constexpr int PL_Q = 4;                                // register-resident 16-byte chunks per thread
constexpr unsigned PL_NO_BIAS = 0xFFFFFFFFu;           // (a NaN pattern: the setters refuse a NaN bias)

// what the kernel reads: the stage's device block (sampler_side.h)
struct LogitParams {
    int top_k;
    int min_p_on;
    float log_min_p;
    float repeat, presence, frequency;
    int last_n;              // 0: no penalty is on
    int n_bias;
    int bias_ids[Q4_MAX_LOGIT_BIAS];
    float bias[Q4_MAX_LOGIT_BIAS];
};

// (the key of a half, a chunk's halves, finish and the block-wide int reductions: logit_block.h)
__device__ __forceinline__ int count_ge(const u32x4& k, unsigned mid) {
    int c = 0;
#pragma unroll
    for (int e = 0; e < 8; e++) c += half_of(k, e) >= mid ? 1 : 0;
    return c;
}
__device__ __forceinline__ int count_eq(const u32x4& k, unsigned T) {
    int c = 0;
#pragma unroll
    for (int e = 0; e < 8; e++) c += half_of(k, e) == T ? 1 : 0;
    return c;
}

// REG: n <= 32 x 1024, the thread's chunks and their keys stay in registers. tokens / pPos null: no window.
template <bool REG, bool ROWS = false>
__global__ void __launch_bounds__(LB_T) logit_process_kernel(q4_half* logits, int n, const LogitParams* __restrict__ prm, const int* tokens,
                                                             const int* pPos, int ld) {
    __shared__ __attribute__((aligned(16))) int s_win[LB_T];
    __shared__ unsigned s_wbias[LB_T];
    __shared__ int red[2][LB_W];
    const int tid = threadIdx.x;
    const int top_k = prm->top_k, min_p_on = prm->min_p_on, n_bias = min(max(prm->n_bias, 0), (int)Q4_MAX_LOGIT_BIAS);
    const int last_n = min(max(prm->last_n, 0), (int)Q4_MAX_PENALTY_WINDOW);
    const float repeat = prm->repeat, presence = prm->presence, frequency = prm->frequency, log_min_p = prm->log_min_p;

    if (ROWS) logits += (size_t)blockIdx.x * ld;

    // ---- steps 1 - 3. The window entry of this thread is requested first (pinned host memory) and used last
    int L = 0, w = -1;
    if (last_n > 0 && tokens != nullptr && pPos != nullptr) {
        const int pos = ROWS ? pPos[blockIdx.x] : *pPos;
        if (pos >= 0 && pos < Q4_MAX_SEQ_LEN) {
            const int start = max(0, pos + 1 - last_n);
            L = pos + 1 - start;                               // (block-uniform, <= 1024)
            if (tid < L) w = tokens[start + tid];
        }
    }
    if (L > 0 || n_bias > 0) {                                 // (block-uniform)
        int bid = -1;
        float bval = 0.f;
        if (tid < n_bias) {
            bid = prm->bias_ids[tid];
            bval = prm->bias[tid];
            if ((unsigned)bid >= (unsigned)n) bid = -1;
        }
        s_wbias[tid] = PL_NO_BIAS;
        if ((unsigned)w >= (unsigned)n) w = -1;
        s_win[tid] = w;                                        // (-1 from L on: it matches no token)
        __syncthreads();
        int cnt = 0, first = -1;
        bool dup = false;
        for (int s = 0; s < L; s += 4) {
            const int4 x = *reinterpret_cast<const int4*>(&s_win[s]);
            const int xs[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
            for (int j = 0; j < 4; j++) {
                cnt += xs[j] == w ? 1 : 0;
                dup = dup || (xs[j] == w && s + j < tid);
                if (xs[j] == bid && first < 0) first = s + j;
            }
        }
        if (bid >= 0 && first >= 0) s_wbias[first] = __float_as_uint(bval);      // (ids are distinct: one writer per slot)
        __syncthreads();
        if (w >= 0 && !dup) {                                  // the first occurrence of a token in the window
            float v = h2f(logits[w]);
            const unsigned b = s_wbias[tid];
            if (b != PL_NO_BIAS) v = v + __uint_as_float(b);
            v = v > 0.f ? v / repeat : v * repeat;
            const float pen = (float)cnt * frequency;
            v = v - (pen + presence);
            logits[w] = finish(v);
        }
        if (bid >= 0 && first < 0) logits[bid] = finish(h2f(logits[bid]) + bval);   // a bias id outside the window
        __syncthreads();                                       // the block's own writes are visible to its loads below
    }
    if (top_k <= 0 && !min_p_on) return;                      // (block-uniform)

    // ---- steps 4 and 5
    const int n8 = n >> 3, nq = REG ? PL_Q : (n8 + LB_T - 1) / LB_T;
    const int tail = n8 * 8 + tid;
    u32x4* lv = reinterpret_cast<u32x4*>(logits);
    u32x4 pq[PL_Q], kk[PL_Q];
    if (REG) {
#pragma unroll
        for (int kq = 0; kq < PL_Q; kq++) {
            const int u = tid + kq * LB_T;
            pq[kq] = u < n8 ? lv[u] : (u32x4){0u, 0u, 0u, 0u};
            kk[kq] = u < n8 ? chunk_keys(pq[kq]) : (u32x4){0u, 0u, 0u, 0u};      // (key 0 is below every threshold the search tries)
        }
    }
    const unsigned th = tail < n ? (unsigned)logits[tail] : 0u;
    const unsigned tkey = tail < n ? half_key(th) : 0u;
    int use = 0;

    // T = the k-th largest key: the largest T with count(key >= T) >= k. lo always has such a count (c_lo), hi never (c_hi)
    const int keff = top_k > 0 ? min(top_k, n) : n;
    int lo = 0, hi = 65536, c_lo = n, c_hi = 0;
    if (keff < n) {
        for (int it = 0; it < 16; it++) {
            const unsigned mid = (unsigned)(lo + hi) >> 1;
            int c = tkey >= mid ? 1 : 0;
#pragma unroll 4
            for (int kq = 0; kq < (REG ? PL_Q : nq); kq++) {
                const int u = tid + kq * LB_T;
                if constexpr (REG) c += count_ge(kk[kq], mid);
                else if (u < n8) c += count_ge(chunk_keys(lv[u]), mid);
            }
            c = block_sum(c, red, use);
            if (c >= keff) { lo = (int)mid; c_lo = c; } else { hi = (int)mid; c_hi = c; }
        }
    }
    const bool all = keff >= n;                                // every entry stays in step 4
    const unsigned T = (unsigned)lo;
    const int need = keff - c_hi;                              // entries equal to T that stay: the first `need` by index
    const bool straddle = !all && c_lo - c_hi > need;

    float m = 0.f;
    if (min_p_on) {
        int mk = (int)tkey;
#pragma unroll 4
        for (int kq = 0; kq < (REG ? PL_Q : nq); kq++) {
            const int u = tid + kq * LB_T;
            u32x4 k;
            if constexpr (REG) k = kk[kq]; else k = u < n8 ? chunk_keys(lv[u]) : (u32x4){0u, 0u, 0u, 0u};
#pragma unroll
            for (int e = 0; e < 8; e++) mk = max(mk, (int)half_of(k, e));
        }
        mk = block_max(mk, red, use);
        m = h2f((uint16_t)key_half((unsigned)mk));
    }

    // the rewrite, row by row in index order (a row: one chunk per thread, 8192 logits; the tail elements last)
    int kept_eq = 0;                                           // entries equal to T in the rows so far (block-uniform; counted only while ties straddle)
    for (int kq = 0; kq <= nq; kq++) {
        const bool is_tail = kq == nq;
        const int u = tid + kq * LB_T;
        const bool have = is_tail ? tail < n : u < n8;
        u32x4 q = {0u, 0u, 0u, 0u}, k = {0u, 0u, 0u, 0u};
        if (is_tail) { q[0] = th; k[0] = tkey; }
        else if (REG) {
#pragma unroll
            for (int j = 0; j < PL_Q; j++) if (j == kq) { q = pq[j]; k = kk[j]; }
        } else if (have) { q = lv[u]; k = chunk_keys(q); }
        const int ne = is_tail ? 1 : 8;
        int base = need;                                       // ties no longer straddle, or the k are full: the rest of the equal entries go
        if (straddle && kept_eq < need) {                      // (block-uniform)
            int mine = 0;
            if (have) mine = is_tail ? (tkey == T ? 1 : 0) : count_eq(k, T);
            int total;
            base = kept_eq + block_scan(mine, red, use, total);
            kept_eq += total;
        }
        if (!have) continue;
        u32x4 o = q;
        bool changed = false;
#pragma unroll
        for (int e = 0; e < 8; e++) {
            if (e < ne) {
                const unsigned h = half_of(q, e), key = half_of(k, e);
                bool keep = all || key > T || (key == T && (!straddle || base++ < need));
                if (keep && min_p_on) keep = h2f((uint16_t)h) - m >= log_min_p;
                if (!keep && h != 0xFC00u) {
                    mask_half(o, e);
                    changed = true;
                }
            }
        }
        if (changed) {
            if (is_tail) logits[tail] = (q4_half)(o[0] & 0xFFFFu);
            else lv[u] = o;
        }
    }
}

// ---- host side: validation, the per-Sampler records, the stage's row ---------------------------------------------------------------------------------
bool finite_f(float v) { return v == v && fabsf(v) != INFINITY; }

bool controls_valid(const q4_sampling_controls* c) {
    return c->top_k >= 0 && c->min_p >= 0.f && c->min_p < 1.f && finite_f(c->repeat_penalty) && c->repeat_penalty > 0.f && finite_f(c->presence_penalty) &&
           finite_f(c->frequency_penalty) && c->penalty_last_n >= 0 && c->penalty_last_n <= Q4_MAX_PENALTY_WINDOW;
}
bool controls_neutral(const q4_sampling_controls* c) {
    return c->top_k == 0 && c->min_p == 0.f && c->repeat_penalty == 1.f && c->presence_penalty == 0.f && c->frequency_penalty == 0.f;
}
// ids distinct and >= 0 (below `limit` where limit > 0); no NaN, no +inf, nothing above 65504 in magnitude except -inf (a ban)
bool bias_valid(const int* ids, const float* bias, int n, int limit) {
    if (n < 0 || n > Q4_MAX_LOGIT_BIAS || (n > 0 && (!ids || !bias))) return false;
    for (int i = 0; i < n; i++) {
        if (ids[i] < 0 || (limit > 0 && ids[i] >= limit)) return false;
        if (bias[i] != bias[i] || bias[i] == INFINITY || (bias[i] != -INFINITY && fabsf(bias[i]) > 65504.0f)) return false;
        for (int j = 0; j < i; j++)
            if (ids[j] == ids[i]) return false;
    }
    return true;
}
void fill_params(LogitParams* P, const q4_sampling_controls* c, const int* ids, const float* bias, int n_bias) {
    memset(P, 0, sizeof(*P));
    P->top_k = c->top_k;
    P->min_p_on = c->min_p > 0.f ? 1 : 0;
    P->log_min_p = c->min_p > 0.f ? logf(c->min_p) : -INFINITY;
    P->repeat = c->repeat_penalty; P->presence = c->presence_penalty; P->frequency = c->frequency_penalty;
    const bool pen = c->repeat_penalty != 1.f || c->presence_penalty != 0.f || c->frequency_penalty != 0.f;
    P->last_n = pen ? c->penalty_last_n : 0;
    P->n_bias = n_bias;
    for (int i = 0; i < n_bias; i++) { P->bias_ids[i] = ids[i]; P->bias[i] = bias[i]; }
}

const q4_sampling_controls NEUTRAL = {0, 0.f, 1.f, 0.f, 0.f, 0};

// what q4_sampler_set_controls / _set_logit_bias keep beside a Sampler (sampler_side.h)
struct Controls : DeviceBlock<LogitParams> {
    q4_sampling_controls c = NEUTRAL;
    int n_bias = 0;
    int ids[Q4_MAX_LOGIT_BIAS];
    float bias[Q4_MAX_LOGIT_BIAS];
    int checked_vocab = -1;            // the vocabulary top_k and the bias ids were last checked against
    bool on() const { return !controls_neutral(&c) || n_bias > 0; }
};
SamplerSides<Controls>& sides() {
    static SamplerSides<Controls> r;
    return r;
}
DeviceBlock<LogitParams> g_op;         // q4_process_logits' own block

int launch(q4_half* logits, int n, const LogitParams* dev, const int* tokens, const int* pPos) {
    if (n <= LB_T * PL_Q * 8) Q4_LAUNCH((logit_process_kernel<true, false>), dim3(1), dim3(LB_T), 0, logits, n, dev, tokens, pPos, 0);
    else Q4_LAUNCH((logit_process_kernel<false, false>), dim3(1), dim3(LB_T), 0, logits, n, dev, tokens, pPos, 0);
    Q4_LAUNCH_CHECK();
    return Q4_OK;
}
// the row form: view the draft view (device), pos_rows the rows' positions (device); both null: no window, as in the step
int launch_rows_of(q4_half* logits, int n, int ld, int n_rows, const LogitParams* dev, const int* view, const int* pos_rows) {
    if (n_rows < 1 || n_rows > PROMPT_PASS_MAX || ld < n || (ld & 7)) return Q4_ERR_ARG;
    if (n <= LB_T * PL_Q * 8) Q4_LAUNCH((logit_process_kernel<true, true>), dim3(n_rows), dim3(LB_T), 0, logits, n, dev, view, pos_rows, ld);
    else Q4_LAUNCH((logit_process_kernel<false, true>), dim3(n_rows), dim3(LB_T), 0, logits, n, dev, view, pos_rows, ld);
    Q4_LAUNCH_CHECK();
    return Q4_OK;
}

// LogitStage::prepare: top_k and the bias ids against this model's vocabulary, then the block
int prepare(const Sampler* sampler, Model*, const Config* p, const void** block) {
    Controls& ctl = sides().of(sampler);
    const int vocab = p->vocab_size;
    if (ctl.checked_vocab != vocab) {
        if (ctl.c.top_k > vocab || !bias_valid(ctl.ids, ctl.bias, ctl.n_bias, vocab)) {
            snprintf(g_last_error, sizeof(g_last_error), "sampling controls: top_k or a logit bias id exceeds the vocabulary (%d)", vocab);
            return Q4_ERR_ARG;
        }
        ctl.checked_vocab = vocab;
    }
    if (ctl.stale()) fill_params(&ctl.host, &ctl.c, ctl.ids, ctl.bias, ctl.n_bias);
    Q4_TRY(ctl.upload());
    *block = ctl.dev;
    return Q4_OK;
}

bool stage_on(const Sampler* sampler, const Model*) { return sides().on(sampler); }
int launch_step(const void* block, const Model*, const Config* p, RunState* s) {
    return launch(s->logits, p->vocab_size, (const LogitParams*)block, &(s->shared_data->tokens[0]), s->pos);
}
int launch_rows(const void* block, const Model*, const Config* p, q4_half* rows, int ld, int n_rows, const int* view, const int* pos_rows) {
    return launch_rows_of(rows, p->vocab_size, ld, n_rows, (const LogitParams*)block, view, pos_rows);
}
const void* stage_block(const Sampler* sampler) { return sides().block(sampler); }
void stage_forget(const Sampler* sampler) { sides().forget(sampler); }

}  // namespace

LogitStage q4::controls_stage = {stage_on, prepare, launch_step, stage_block, stage_forget, launch_rows};

extern "C" {

int q4_sampler_set_controls(Sampler* sampler, const q4_sampling_controls* controls) {
    if (!sampler || (controls && !controls_valid(controls))) return Q4_ERR_ARG;
    if (!controls && !sides().find(sampler)) return Q4_OK;     // off, and never on
    Controls& ctl = sides().of(sampler);
    const int keep_n = ctl.c.penalty_last_n;
    ctl.c = controls ? *controls : NEUTRAL;
    if (!controls) ctl.c.penalty_last_n = keep_n;
    ctl.dirty = true;
    ctl.checked_vocab = -1;
    return Q4_OK;
}
int q4_sampler_get_controls(const Sampler* sampler, q4_sampling_controls* out) {
    if (!sampler || !out) return Q4_ERR_ARG;
    const Controls* ctl = sides().find(sampler);
    *out = ctl ? ctl->c : NEUTRAL;
    return Q4_OK;
}
int q4_sampler_set_logit_bias(Sampler* sampler, const int* ids, const float* bias, int n) {
    if (!sampler || !bias_valid(ids, bias, n, 0)) return Q4_ERR_ARG;
    if (n == 0 && !sides().find(sampler)) return Q4_OK;
    Controls& ctl = sides().of(sampler);
    ctl.n_bias = n;
    for (int i = 0; i < n; i++) { ctl.ids[i] = ids[i]; ctl.bias[i] = bias[i]; }
    ctl.dirty = true;
    ctl.checked_vocab = -1;
    return Q4_OK;
}

// "top_k=40,min_p=0.05,repeat_penalty=1.1,last_n=64,presence=0,frequency=0": any subset, any order; a key that is left out keeps its neutral value
// (last_n: 64). An unknown key, a key without a value, a number with trailing text or a value the setter would refuse: Q4_ERR_ARG, *out untouched.
int q4_parse_sampling_controls(const char* text, q4_sampling_controls* out) {
    if (!text || !out) return Q4_ERR_ARG;
    q4_sampling_controls c = NEUTRAL;
    c.penalty_last_n = 64;
    const char* p = text;
    while (*p) {
        char key[OPTION_KEY_CAP], val[64];
        if (!next_option(&p, key, val, sizeof(val))) return Q4_ERR_ARG;
        char* rest = nullptr;
        if (!strcmp(key, "top_k") || !strcmp(key, "last_n")) {
            const long v = strtol(val, &rest, 10);
            if (*rest || v < -1000000 || v > 1000000) return Q4_ERR_ARG;
            (!strcmp(key, "top_k") ? c.top_k : c.penalty_last_n) = (int)v;
        } else {
            float* f = !strcmp(key, "min_p") ? &c.min_p : !strcmp(key, "repeat_penalty") ? &c.repeat_penalty : !strcmp(key, "presence") ? &c.presence_penalty :
                       !strcmp(key, "frequency") ? &c.frequency_penalty : nullptr;
            if (!f) return Q4_ERR_ARG;
            *f = strtof(val, &rest);
            if (*rest || rest == val) return Q4_ERR_ARG;
        }
    }
    if (!controls_valid(&c)) return Q4_ERR_ARG;
    *out = c;
    return Q4_OK;
}

int q4_process_logits(q4_half* logits, int n, const q4_sampling_controls* controls, const int* bias_ids, const float* bias, int n_bias, const int* tokens,
                      const int* pPos) {
    if (!logits || n < 1 || !controls || !controls_valid(controls) || controls->top_k > n || !bias_valid(bias_ids, bias, n_bias, n)) return Q4_ERR_ARG;
    if (controls_neutral(controls) && n_bias == 0) return Q4_OK;
    fill_params(&g_op.host, controls, bias_ids, bias, n_bias);
    g_op.dirty = true;
    Q4_TRY(g_op.upload());
    return launch(logits, n, g_op.dev, tokens, pPos);
}
int q4_process_logits_rows(q4_half* logits, int n, const q4_sampling_controls* controls, const int* bias_ids, const float* bias, int n_bias, int ld,
                           int n_rows, const int* tokens_view_dev, const int* pos_rows_dev) {
    if (!logits || n < 1 || !controls || !controls_valid(controls) || controls->top_k > n || !bias_valid(bias_ids, bias, n_bias, n)) return Q4_ERR_ARG;
    if (n_rows < 1 || n_rows > PROMPT_PASS_MAX || ld < n || (ld & 7)) return Q4_ERR_ARG;
    if (controls_neutral(controls) && n_bias == 0) return Q4_OK;
    fill_params(&g_op.host, controls, bias_ids, bias, n_bias);
    g_op.dirty = true;
    Q4_TRY(g_op.upload());
    return launch_rows_of(logits, n, ld, n_rows, g_op.dev, tokens_view_dev, pos_rows_dev);
}

}  // extern "C"
