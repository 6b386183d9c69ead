// q4_dry.hip -- the DRY ("don't repeat yourself") penalty and the no-repeat-n-gram ban as ONE launch that rewrites the step's fp16 logits in place,
// behind the guide's launch and in front of the sampling controls' launch. Not in the reference. The rule is written down in llama2_q4.h.
// ONE 1024-thread block; thread t owns the window entries 4t .. 4t + 3 (index order is thread order), the window lives in LDS.
//   1. the ring is requested first (pinned host memory, at most 16 KB); the parameter block is staged while the request is in flight.
//   2. R, the run of non-breaker entries that ends at ring[p]: one block-wide maximum over the positions of the breakers (a vocabulary bitmap).
//   3. the candidates -- window slots in front of the last whose token equals ring[p] -- are compacted in index order with one block prefix sum.
//   4. candidate c goes to thread c mod 1024: it walks back at most 64 LDS entries (its match length M) and reads the token behind it.
//   5. the per-token maximum over the COMPACTED list only (key = M * 4096 + 4095 - c: the largest M, then the first in index order): the one candidate
//      of a token that no other beats rewrites that token's logit -- the ban, or one fp32 subtraction of pen[min(M, R)] finished by
//      logit_block.h's finish. One writer per logit: no atomics, no arrival order, the same input gives the same bytes on every launch.
// The vocabulary is never scanned: the cost does not depend on n. Worst case, a window of one repeated token: 4095 candidates, every M 64, 4095 x 4
// comparisons per thread over broadcast 16-byte LDS reads. No ring entry or breaker id indexes anything before it has been checked against [0, n).
// The row form (ROWS; a verify pass with q4_set_pass_stages on, q4_dry_penalty_rows): block r of up to PROMPT_PASS_MAX is row r -- its logits `ld` halves
// behind row 0's, its position pPos[r], and `tokens` is the pass's draft view (by absolute position: the ring up to the pass's first position, the drafts
// behind it), not the pinned ring. Everything between those three substitutions is the step's one body.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <map>
#include <vector>
#include "q4_device.h"
#include "q4_model.h"
#include "sampler_side.h"
#include "logit_block.h"
#include "option_text.h"
#include "prompt_pass.h"
#pragma clang fp contract(off)
using namespace q4;

namespace {

constexpr int DR_E = 4;                                // window entries per thread
constexpr int DR_CAP = Q4_DRY_MAX_MATCH;
static_assert(LB_T * DR_E == Q4_MAX_DRY_WINDOW, "four window entries per thread");

// what the kernel reads: the stage's device block (sampler_side.h)
struct DryParams {
    int last_n;              // 0: off
    int allowed;             // allowed_length
    int ngram;               // no_repeat_ngram_size, 0: no ban
    int dry_on;              // multiplier > 0
    int breaker_words;       // 32-bit words of the bitmap below, 0: no breakers
    int pad;
    const unsigned* breakers;    // bit i: token i is a breaker
    float pen[DR_CAP + 1];   // q4_dry_penalty_table
};

// (finish and the block-wide int reductions: logit_block.h)
template <bool ROWS = false>
__global__ void __launch_bounds__(LB_T) dry_kernel(q4_half* logits, int n, const DryParams* __restrict__ prm, const int* tokens, const int* pPos, int ld) {
    __shared__ __attribute__((aligned(16))) int s_win[LB_T * DR_E];      // the window, local index k = ring index - start
    __shared__ __attribute__((aligned(16))) int s_tok[LB_T * DR_E];      // per candidate: the token behind it, -1: outside [0, n)
    __shared__ __attribute__((aligned(16))) int s_key[LB_T * DR_E];      // per candidate: its slot k, then M * 4096 + 4095 - c
    __shared__ float s_pen[DR_CAP + 1];
    __shared__ int red[2][LB_W];
    const int tid = threadIdx.x;
    const int last_n = min(max(prm->last_n, 0), (int)Q4_MAX_DRY_WINDOW);
    if (last_n == 0 || tokens == nullptr || pPos == nullptr) return;   // (block-uniform, like every return below)
    const int pos = ROWS ? pPos[blockIdx.x] : *pPos;
    if (ROWS) logits += (size_t)blockIdx.x * ld;
    if (pos < 1 || pos >= Q4_MAX_SEQ_LEN) return;                      // (position 0: a window of one entry has no candidate)
    const int start = max(0, pos + 1 - last_n);
    const int L = pos + 1 - start;                                     // 1 .. 4096
    if (L < 2) return;

    // ---- 1. the ring first, the parameters while it is in flight
    int w[DR_E];
#pragma unroll
    for (int j = 0; j < DR_E; j++) {
        const int k = tid * DR_E + j;
        w[j] = k < L ? tokens[start + k] : 0;
    }
    const int allowed = prm->allowed, ngram = prm->ngram, dry_on = prm->dry_on, words = prm->breakers ? prm->breaker_words : 0;
    const unsigned* __restrict__ bits = prm->breakers;
    if (tid <= DR_CAP) s_pen[tid] = prm->pen[tid];

    // ---- 2. the window into LDS; R from the last breaker's position
    int bk = -1;
#pragma unroll
    for (int j = 0; j < DR_E; j++) {
        const int k = tid * DR_E + j, t = w[j];
        if (k < L && (unsigned)t < (unsigned)n && (t >> 5) < words && ((bits[t >> 5] >> (t & 31)) & 1u)) bk = k;
    }
    *reinterpret_cast<int4*>(&s_win[tid * DR_E]) = make_int4(w[0], w[1], w[2], w[3]);
    int use = 0;
    bk = block_max(bk, red, use);                                      // (its barrier publishes s_win and s_pen)
    const int R = min(DR_CAP, L - 1 - bk);
    const bool ban_on = ngram >= 2;
    if (!ban_on && (!dry_on || R < allowed)) return;                   // nothing can be touched
    const int last = s_win[L - 1];

    // ---- 3. the candidates, compacted in index order
    int mine = 0;
#pragma unroll
    for (int j = 0; j < DR_E; j++) mine += (tid * DR_E + j < L - 1 && w[j] == last) ? 1 : 0;
    int C;
    int at = block_scan(mine, red, use, C);
    if (C == 0) return;
#pragma unroll
    for (int j = 0; j < DR_E; j++)
        if (tid * DR_E + j < L - 1 && w[j] == last) s_key[at++] = tid * DR_E + j;
    __syncthreads();

    // ---- 4. candidate c = tid + i * 1024: its match length and the token behind it
    const int Cpad = (C + 3) & ~3;
    int myt[DR_E], mykey[DR_E];
#pragma unroll
    for (int i = 0; i < DR_E; i++) {
        const int c = tid + i * LB_T;
        myt[i] = -1;
        mykey[i] = 0;
        if (c < C) {
            const int k = s_key[c];                                    // 0 <= k <= L - 2
            int M = 1;
            while (M < DR_CAP && k - M >= 0 && s_win[k - M] == s_win[L - 1 - M]) M++;
            int t = s_win[k + 1];
            if ((unsigned)t >= (unsigned)n) t = -1;
            myt[i] = t;
            mykey[i] = M * (LB_T * DR_E) + (LB_T * DR_E - 1 - c);
        }
        if (c < Cpad) {                                                // (slot c was read by this thread alone)
            s_tok[c] = myt[i];
            s_key[c] = mykey[i];
        }
    }
    __syncthreads();

    // ---- 5. the candidate of a token that no other candidate of that token beats rewrites its logit
    bool lose[DR_E] = {false, false, false, false};
    if (tid < C) {
        const int mine_n = min(DR_E, (C - tid + LB_T - 1) / LB_T);     // this thread's candidates
        for (int s = 0; s < Cpad; s += 4) {
            const int4 T = *reinterpret_cast<const int4*>(&s_tok[s]);
            const int4 K = *reinterpret_cast<const int4*>(&s_key[s]);
#pragma unroll
            for (int i = 0; i < DR_E; i++)
                if (i < mine_n)
                    lose[i] = lose[i] || (T.x == myt[i] && K.x > mykey[i]) || (T.y == myt[i] && K.y > mykey[i]) || (T.z == myt[i] && K.z > mykey[i]) ||
                              (T.w == myt[i] && K.w > mykey[i]);
        }
    }
#pragma unroll
    for (int i = 0; i < DR_E; i++) {
        const int t = myt[i];
        if (t < 0 || lose[i]) continue;
        const int M = mykey[i] / (LB_T * DR_E);
        if (ban_on && M >= ngram - 1) logits[t] = (q4_half)0xFC00u;
        else if (dry_on) {
            const int Lt = min(M, R);
            if (Lt >= allowed) logits[t] = finish(h2f(logits[t]) - s_pen[Lt]);
        }
    }
}

// ---- host side: validation, the per-Sampler records, the stage's row ---------------------------------------------------------------------------------
const q4_dry_controls DRY_DEFAULT = {0.f, 1.75f, 2, 1024, 0};

bool finite_f(float v) { return v == v && fabsf(v) != INFINITY; }
bool dry_valid(const q4_dry_controls* c) {
    return finite_f(c->multiplier) && c->multiplier >= 0.f && finite_f(c->base) && c->base >= 1.f && c->allowed_length >= 1 &&
           c->allowed_length <= Q4_DRY_MAX_MATCH && c->last_n >= 0 && c->last_n <= Q4_MAX_DRY_WINDOW &&
           (c->no_repeat_ngram_size == 0 || (c->no_repeat_ngram_size >= 2 && c->no_repeat_ngram_size <= Q4_DRY_MAX_MATCH + 1));
}
bool dry_off(const q4_dry_controls* c) { return (c->multiplier == 0.f && c->no_repeat_ngram_size == 0) || c->last_n == 0; }
// ids distinct and >= 0 (below `limit` where limit > 0)
bool breakers_valid(const int* ids, int n, int limit) {
    if (n < 0 || (n > 0 && !ids)) return false;
    std::vector<int> sorted(ids, ids + n);
    std::sort(sorted.begin(), sorted.end());
    for (int i = 0; i < n; i++)
        if (sorted[i] < 0 || (limit > 0 && sorted[i] >= limit) || (i > 0 && sorted[i] == sorted[i - 1])) return false;
    return true;
}
void penalty_table(const q4_dry_controls* c, float* out) {
    for (int L = 0; L <= Q4_DRY_MAX_MATCH; L++) {
        float v = 0.f;
        if (L >= c->allowed_length && c->multiplier > 0.f) {
            v = c->multiplier * powf(c->base, (float)(L - c->allowed_length));
            if (!(v <= 3.0e38f)) v = 3.0e38f;
        }
        out[L] = v;
    }
}
void fill_params(DryParams* P, const q4_dry_controls* c, const unsigned* bitmap, int words) {
    memset(P, 0, sizeof(*P));
    P->last_n = dry_off(c) ? 0 : c->last_n;
    P->allowed = c->allowed_length;
    P->ngram = c->no_repeat_ngram_size;
    P->dry_on = c->multiplier > 0.f ? 1 : 0;
    P->breaker_words = bitmap ? words : 0;
    P->breakers = bitmap;
    penalty_table(c, P->pen);
}

// the device block and the breaker bitmap it points at
struct DeviceSide : DeviceBlock<DryParams> {
    std::vector<unsigned> bitmap_host;
    unsigned* bitmap = nullptr;
    int bitmap_words = 0;              // allocated
    void release() {
        DeviceBlock<DryParams>::release();
        if (bitmap) (void)hipFree(bitmap);
        bitmap = nullptr; bitmap_words = 0;
    }
};
// The bitmap for a vocabulary of `vocab` tokens and the block, uploaded in stream order. The bitmap grows only after the stream has drained: a launch
// in flight may still read the old one.
int upload(DeviceSide& d, const q4_dry_controls* c, const std::vector<int>& breakers, int vocab) {
    const int words = breakers.empty() ? 0 : (vocab + 31) / 32;
    if (words > d.bitmap_words) {
        Q4_HIP(hipStreamSynchronize(g_stream));
        if (d.bitmap) (void)hipFree(d.bitmap);
        d.bitmap = nullptr; d.bitmap_words = 0;
        Q4_HIP(hipMalloc((void**)&d.bitmap, (size_t)words * sizeof(unsigned)));
        d.bitmap_words = words;
    }
    if (words) {
        d.bitmap_host.assign((size_t)words, 0u);
        for (int id : breakers) d.bitmap_host[(size_t)id >> 5] |= 1u << (id & 31);
        Q4_HIP(hipMemcpyAsync(d.bitmap, d.bitmap_host.data(), (size_t)words * sizeof(unsigned), hipMemcpyHostToDevice, g_stream));
    }
    fill_params(&d.host, c, words ? d.bitmap : nullptr, words);
    d.dirty = true;
    return d.upload();
}

// what q4_sampler_set_dry / _set_dry_breakers keep beside a Sampler (sampler_side.h)
struct Dry : DeviceSide {
    q4_dry_controls c = DRY_DEFAULT;
    std::vector<int> breakers;
    int vocab = -1;                    // the vocabulary the breaker ids were last checked against and the bitmap was built for
    bool on() const { return !dry_off(&c); }
};
SamplerSides<Dry>& sides() {
    static SamplerSides<Dry> r;
    return r;
}
DeviceSide g_op;                       // q4_dry_penalty's own block and bitmap

int launch(q4_half* logits, int n, const DryParams* dev, const int* tokens, const int* pPos) {
    Q4_LAUNCH(dry_kernel<false>, dim3(1), dim3(LB_T), 0, logits, n, dev, tokens, pPos, 0);
    Q4_LAUNCH_CHECK();
    return Q4_OK;
}
// the row form: view the draft view (device), pos_rows the rows' positions (device)
int launch_rows_of(q4_half* logits, int n, int ld, int n_rows, const DryParams* dev, const int* view, const int* pos_rows) {
    if (n_rows < 1 || n_rows > PROMPT_PASS_MAX || ld < n || (ld & 7)) return Q4_ERR_ARG;
    Q4_LAUNCH(dry_kernel<true>, dim3(n_rows), dim3(LB_T), 0, logits, n, dev, view, pos_rows, ld);
    Q4_LAUNCH_CHECK();
    return Q4_OK;
}

// LogitStage::prepare: the breaker ids against this model's vocabulary, then the bitmap and the block
int prepare(const Sampler* sampler, Model*, const Config* p, const void** block) {
    Dry& r = sides().of(sampler);
    const int vocab = p->vocab_size;
    if (r.vocab != vocab) {
        if (!breakers_valid(r.breakers.data(), (int)r.breakers.size(), vocab)) {
            snprintf(g_last_error, sizeof(g_last_error), "DRY: a breaker id exceeds the vocabulary (%d)", vocab);
            return Q4_ERR_ARG;
        }
        r.vocab = vocab;
        r.dirty = true;
    }
    if (r.stale()) Q4_TRY(upload(r, &r.c, r.breakers, vocab));
    *block = r.dev;
    return Q4_OK;
}

bool stage_on(const Sampler* sampler, const Model*) { return sides().on(sampler); }
int launch_step(const void* block, const Model*, const Config* p, RunState* s) {
    return launch(s->logits, p->vocab_size, (const DryParams*)block, &(s->shared_data->tokens[0]), s->pos);
}
int launch_rows(const void* block, const Model*, const Config* p, q4_half* rows, int ld, int n_rows, const int* view, const int* pos_rows) {
    return launch_rows_of(rows, p->vocab_size, ld, n_rows, (const DryParams*)block, view, pos_rows);
}
const void* stage_block(const Sampler* sampler) { return sides().block(sampler); }
void stage_forget(const Sampler* sampler) { sides().forget(sampler); }

}  // namespace

LogitStage q4::dry_stage = {stage_on, prepare, launch_step, stage_block, stage_forget, launch_rows};

extern "C" {

int q4_sampler_set_dry(Sampler* sampler, const q4_dry_controls* controls) {
    if (!sampler || (controls && !dry_valid(controls))) return Q4_ERR_ARG;
    if (!controls && !sides().find(sampler)) return Q4_OK;     // off, and never on
    Dry& r = sides().of(sampler);
    r.c = controls ? *controls : DRY_DEFAULT;
    r.dirty = true;
    return Q4_OK;
}
int q4_sampler_get_dry(const Sampler* sampler, q4_dry_controls* out) {
    if (!sampler || !out) return Q4_ERR_ARG;
    const Dry* r = sides().find(sampler);
    *out = r ? r->c : DRY_DEFAULT;
    return Q4_OK;
}
int q4_sampler_set_dry_breakers(Sampler* sampler, const int* ids, int n) {
    if (!sampler || !breakers_valid(ids, n, 0)) return Q4_ERR_ARG;
    if (n == 0 && !sides().find(sampler)) return Q4_OK;
    Dry& r = sides().of(sampler);
    r.breakers.assign(ids, ids + n);
    r.dirty = true;
    r.vocab = -1;
    return Q4_OK;
}

// "multiplier=0.8,base=1.75,allowed=2,last_n=1024,ngram=0": any subset, any order; a key that is left out keeps its default (those values, multiplier
// 0). An unknown key, a key without a value, a number with trailing text or a value the setter would refuse: Q4_ERR_ARG, *out untouched.
int q4_parse_dry(const char* text, q4_dry_controls* out) {
    if (!text || !out) return Q4_ERR_ARG;
    q4_dry_controls c = DRY_DEFAULT;
    const char* p = text;
    while (*p) {
        char key[OPTION_KEY_CAP], val[64];
        if (!next_option(&p, key, val, sizeof(val))) return Q4_ERR_ARG;
        char* rest = nullptr;
        int* iv = !strcmp(key, "allowed") ? &c.allowed_length : !strcmp(key, "last_n") ? &c.last_n : !strcmp(key, "ngram") ? &c.no_repeat_ngram_size : nullptr;
        if (iv) {
            const long v = strtol(val, &rest, 10);
            if (*rest || rest == val || v < -1000000 || v > 1000000) return Q4_ERR_ARG;
            *iv = (int)v;
        } else {
            float* f = !strcmp(key, "multiplier") ? &c.multiplier : !strcmp(key, "base") ? &c.base : nullptr;
            if (!f) return Q4_ERR_ARG;
            *f = strtof(val, &rest);
            if (*rest || rest == val) return Q4_ERR_ARG;
        }
    }
    if (!dry_valid(&c)) return Q4_ERR_ARG;
    *out = c;
    return Q4_OK;
}

int q4_dry_penalty_table(const q4_dry_controls* controls, float out[65]) {
    if (!controls || !out || !dry_valid(controls)) return Q4_ERR_ARG;
    penalty_table(controls, out);
    return Q4_OK;
}

int q4_dry_penalty(q4_half* logits, int n, const q4_dry_controls* controls, const int* breaker_ids, int n_breakers, const int* tokens, const int* pPos) {
    if (!logits || n < 1 || !controls || !dry_valid(controls) || !breakers_valid(breaker_ids, n_breakers, n)) return Q4_ERR_ARG;
    if (dry_off(controls) || !tokens || !pPos) return Q4_OK;
    Q4_TRY(upload(g_op, controls, std::vector<int>(breaker_ids, breaker_ids + n_breakers), n));
    return launch(logits, n, g_op.dev, tokens, pPos);
}
int q4_dry_penalty_rows(q4_half* logits, int n, const q4_dry_controls* controls, const int* breaker_ids, int n_breakers, int ld, int n_rows,
                        const int* tokens_view_dev, const int* pos_rows_dev) {
    if (!logits || n < 1 || !controls || !dry_valid(controls) || !breakers_valid(breaker_ids, n_breakers, n)) return Q4_ERR_ARG;
    if (n_rows < 1 || n_rows > PROMPT_PASS_MAX || ld < n || (ld & 7)) return Q4_ERR_ARG;
    if (dry_off(controls) || !tokens_view_dev || !pos_rows_dev) return Q4_OK;
    Q4_TRY(upload(g_op, controls, std::vector<int>(breaker_ids, breaker_ids + n_breakers), n));
    return launch_rows_of(logits, n, ld, n_rows, g_op.dev, tokens_view_dev, pos_rows_dev);
}

}  // extern "C"
