// q4_adaptive.hip -- the three truncation rules that take their threshold from a statistic of the whole distribution: top-n-sigma, typical-p and
// Mirostat v2, as ONE launch that masks the step's fp16 logits in place, behind the sampling controls' launch and in front of the argmax or the
// sampler. Not in the reference. The rule is written down in llama2_q4.h.
// ONE 1024-thread block, the partition of logit_block.h: thread t owns the 16-byte chunks t, t + 1024, ... and, past the last whole chunk, one tail
// element; up to 32 x 1024 logits stay in registers across the stages, larger vocabularies are read again from L2 in every pass. A masked entry IS the
// half -inf from then on: a later stage sees it as an entry that takes no part.
//   every statistic is a sum in ONE fixed order, that of q4_logprobs.hip: a thread adds its elements in ascending index in runs of 32 (four chunks),
//   adds the runs' totals in ascending order, then its tail element; a 64-lane tree (wave_sum); a 16-lane tree over the wave totals (row16_sum). An
//   entry that takes no part adds 0. No atomics, no arrival order: the same input gives the same bytes on every launch.
//   1. top-n-sigma: three reductions (the maximum; sum and count; the squared deviations), one masking pass, no expf.
//   2. typical-p: the maximum, the sum of exponentials, {H, the whole mass} and the largest deviation (four reductions); then d*, the smallest
//      deviation whose tier completes the mass, by a binary search on the deviation's fp32 bit pattern (non-negative: a monotone key) with ONE
//      block-wide weighted sum per round, at most 31 rounds; p_i and the key stay in registers, so a round is 33 compares and adds per thread.
//   3. Mirostat v2: the chain p -> tokens[p] (pinned host memory, requested first) -> side[tok] gives mu_p; the maximum, the sum of exponentials at
//      the sampler's temperature, one masking pass, one pass that writes the kept entries' w to the side buffer and sums their exponentials again.
// An off stage costs no pass. Nothing that comes out of memory indexes anything unchecked: p against [0, seq_len), tokens[p] against [0, n).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include <map>
#include <vector>
#include "q4_device.h"
#include "q4_model.h"
#include "sampler_side.h"
#include "logit_block.h"
#include "option_text.h"
#pragma clang fp contract(off)
using namespace q4;

namespace {

constexpr int AD_Q = 4;                                // register-resident 16-byte chunks per thread
constexpr int AD_SLOTS = AD_Q * 8 + 1;                 // a thread's elements in the register form: 32 and the tail
constexpr int AD_REC = Q4_ADAPTIVE_RECORD;
constexpr float AD_LOG2E = 1.44269504088896340736f, AD_LN2 = 0.69314718055994530942f;

// what the kernel reads: the stage's device block (sampler_side.h)
struct AdaptiveParams {
    float typical_p;         // >= 1: off
    float top_n_sigma;       // 0: off
    float tau, eta;          // tau 0: Mirostat off
    float temperature;       // the sampler's, Mirostat only
    int pad[3];
};

__device__ __forceinline__ bool takes_part(unsigned h) { return (h & 0x7FFFu) < 0x7C00u; }      // a finite half

// the thread's view of the logits
struct View {
    u32x4 pq[AD_Q];          // REG: the thread's chunks
    unsigned th;             // the tail element (0xFC00: none)
    unsigned dirty;          // REG: bit kq -- chunk kq changed; bit AD_Q: the tail changed
    u32x4* lv;
    int n, n8, nq, tail, tid;
};

// f(slot, index, half) for every element of the thread in ascending index; slot: kq * 8 + e in the register form (a constant once unrolled), 32: the tail
template <bool REG, class F>
__device__ __forceinline__ void each(const View& c, F f) {
    if constexpr (REG) {
#pragma unroll
        for (int kq = 0; kq < AD_Q; kq++) {
            const int u = c.tid + kq * LB_T;
            if (u < c.n8) {
#pragma unroll
                for (int e = 0; e < 8; e++) f(kq * 8 + e, u * 8 + e, half_of(c.pq[kq], e));
            }
        }
    } else {
        for (int kq = 0; kq < c.nq; kq++) {
            const int u = c.tid + kq * LB_T;
            if (u < c.n8) {
                const u32x4 q = c.lv[u];
#pragma unroll
                for (int e = 0; e < 8; e++) f(0, u * 8 + e, half_of(q, e));
            }
        }
    }
    if (c.tail < c.n) f(AD_SLOTS - 1, c.tail, c.th);
}
// the thread's part of a sum in the fixed order of the header: f(slot, index, half) is the element's term
template <bool REG, class F>
__device__ __forceinline__ float thread_sum(const View& c, F f) {
    float total = 0.f, run = 0.f;
    if constexpr (REG) {
#pragma unroll
        for (int kq = 0; kq < AD_Q; kq++) {
            const int u = c.tid + kq * LB_T;
            if (u < c.n8) {
#pragma unroll
                for (int e = 0; e < 8; e++) run += f(kq * 8 + e, u * 8 + e, half_of(c.pq[kq], e));
            }
        }
        total += run;                                          // one run of 32
    } else {
        for (int kq = 0; kq < c.nq; kq++) {
            const int u = c.tid + kq * LB_T;
            if (u < c.n8) {
                const u32x4 q = c.lv[u];
#pragma unroll
                for (int e = 0; e < 8; e++) run += f(0, u * 8 + e, half_of(q, e));
            }
            if ((kq & (AD_Q - 1)) == AD_Q - 1) { total += run; run = 0.f; }
        }
        if (c.nq & (AD_Q - 1)) total += run;                   // the last, shorter run
    }
    if (c.tail < c.n) total += f(AD_SLOTS - 1, c.tail, c.th);
    return total;
}
// every entry that takes part and that keep(slot, index, half) refuses becomes -inf
template <bool REG, class F>
__device__ __forceinline__ void mask_pass(View& c, F keep) {
    if constexpr (REG) {
#pragma unroll
        for (int kq = 0; kq < AD_Q; kq++) {
            const int u = c.tid + kq * LB_T;
            if (u < c.n8) {
#pragma unroll
                for (int e = 0; e < 8; e++) {
                    const unsigned h = half_of(c.pq[kq], e);
                    if (takes_part(h) && !keep(kq * 8 + e, u * 8 + e, h)) { mask_half(c.pq[kq], e); c.dirty |= 1u << kq; }
                }
            }
        }
    } else {
        for (int kq = 0; kq < c.nq; kq++) {
            const int u = c.tid + kq * LB_T;
            if (u < c.n8) {
                const u32x4 q = c.lv[u];
                u32x4 o = q;
                bool changed = false;
#pragma unroll
                for (int e = 0; e < 8; e++) {
                    const unsigned h = half_of(q, e);
                    if (takes_part(h) && !keep(0, u * 8 + e, h)) { mask_half(o, e); changed = true; }
                }
                if (changed) c.lv[u] = o;                      // (the thread reads its own chunks only: program order is enough)
            }
        }
    }
    if (c.tail < c.n && takes_part(c.th) && !keep(AD_SLOTS - 1, c.tail, c.th)) { c.th = 0xFC00u; c.dirty |= 1u << AD_Q; }
}

// Block-wide reductions. `use` counts the calls: two LDS rows take turns, so ONE barrier per call is enough (a row is written again only two calls
// later, behind the barrier of the call in between, which every thread passes after its reads). Every thread gets the result.
template <int N>
__device__ __forceinline__ void block_sum(float (&v)[N], float (*red)[2 * LB_W], int& use) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float* row = red[use++ & 1];
#pragma unroll
    for (int i = 0; i < N; i++) {
        v[i] = wave_sum(v[i]);
        if (lane == 0) row[i * LB_W + wave] = v[i];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < N; i++) v[i] = row16_sum(row[i * LB_W + (lane & 15)]);
}
__device__ __forceinline__ float block_sum1(float v, float (*red)[2 * LB_W], int& use) {
    float a[1] = {v};
    block_sum<1>(a, red, use);
    return a[0];
}
__device__ __forceinline__ float block_max(float v, float (*red)[2 * LB_W], int& use) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float* row = red[use++ & 1];
    v = wave_max(v);
    if (lane == 0) row[wave] = v;
    __syncthreads();
    return row16_max(row[lane & 15]);
}
// the largest value among the entries that take part, -inf: none
template <bool REG>
__device__ __forceinline__ float view_max(const View& c, float (*red)[2 * LB_W], int& use) {
    float m = -INFINITY;
    each<REG>(c, [&](int, int, unsigned h) { if (takes_part(h)) m = fmaxf(m, h2f((uint16_t)h)); });
    return block_max(m, red, use);
}

// REG: n <= 32 x 1024. mu_ring / side / tokens / pPos null: no Mirostat. rec: AD_REC floats per record, record *pPos when rec_by_pos, else record 0.
template <bool REG>
__global__ void __launch_bounds__(LB_T) adaptive_kernel(q4_half* logits, int n, const AdaptiveParams* __restrict__ prm, float* mu_ring, float* side,
                                                        float* rec, int rec_by_pos, int seq_len, const int* tokens, const int* pPos) {
    __shared__ float red[2][2 * LB_W];
    int (*const ired)[2 * LB_W] = reinterpret_cast<int (*)[2 * LB_W]>(red);     // the same two rows for logit_block.h's int maximum
    const int tid = threadIdx.x;
    const float typical_p = prm->typical_p, nsigma = prm->top_n_sigma, tau = prm->tau, eta = prm->eta, temp = prm->temperature;
    const bool miro = tau > 0.f && temp > 0.f && mu_ring != nullptr && side != nullptr && tokens != nullptr && pPos != nullptr;
    const int p = pPos ? *pPos : 0;
    if (p < 0 || p >= seq_len) return;                         // (block-uniform, like every branch on a statistic below)

    // ---- Mirostat's chain first: the ring entry crosses PCIe. ONE thread resolves it -- one request, not sixteen waves' -- and hands mu_p to the
    // block through LDS behind the first barrier of stage 3; its reads of the side buffer are complete before that barrier, the block's stores to the
    // side buffer come behind it
    __shared__ float s_mu;
    const float none = __uint_as_float(0xFFFFFFFFu);
    float mu_p = none;
    if (miro && tid == 0) {
        const int tok = tokens[p];
        const float prev = p > 0 ? mu_ring[p - 1] : none;
        const int side_pos = __float_as_int(side[n]);
        const float side_lse = side[n + 1];
        const float side_tok = (unsigned)tok < (unsigned)n ? side[tok] : -INFINITY;
        if (prev != prev) mu_p = 2.f * tau;                    // a span starts
        else if (side_pos == p - 1 && side_tok == side_tok && fabsf(side_tok) != INFINITY) {
            const float surprise = (side_lse - side_tok) * AD_LOG2E;
            const float over = surprise - tau;
            mu_p = prev - eta * over;
        } else mu_p = prev;                                    // a rewind: the side buffer describes another position
        s_mu = mu_p;
    }

    View c;
    c.n = n; c.n8 = n >> 3; c.nq = REG ? AD_Q : (c.n8 + LB_T - 1) / LB_T; c.tail = c.n8 * 8 + tid; c.tid = tid; c.dirty = 0u;
    c.lv = reinterpret_cast<u32x4*>(logits);
#pragma unroll
    for (int kq = 0; kq < AD_Q; kq++) {
        const int u = tid + kq * LB_T;
        c.pq[kq] = (REG && u < c.n8) ? c.lv[u] : (u32x4){0xFC00FC00u, 0xFC00FC00u, 0xFC00FC00u, 0xFC00FC00u};
    }
    c.th = c.tail < n ? (unsigned)logits[c.tail] : 0xFC00u;
    int use = 0;
    float r_ts = none, r_h = none, r_d = none, r_tm = none, r_lse = none, r_lset = none;

    // ---- 1. top-n-sigma
    if (nsigma > 0.f) {
        const float m = view_max<REG>(c, red, use);
        if (m != -INFINITY) {
            float a[2];
            a[0] = thread_sum<REG>(c, [&](int, int, unsigned h) { return takes_part(h) ? h2f((uint16_t)h) : 0.f; });
            a[1] = thread_sum<REG>(c, [&](int, int, unsigned h) { return takes_part(h) ? 1.f : 0.f; });
            block_sum<2>(a, red, use);
            const float cnt = a[1], mean = a[0] / cnt;
            const float sq = block_sum1(thread_sum<REG>(c, [&](int, int, unsigned h) {
                const float d = h2f((uint16_t)h) - mean;
                return takes_part(h) ? d * d : 0.f;
            }), red, use);
            const float sigma = sqrtf(sq / cnt);
            const float T_s = m - nsigma * sigma;
            r_ts = T_s;
            mask_pass<REG>(c, [&](int, int, unsigned h) { return h2f((uint16_t)h) >= T_s; });
        }
    }

    // ---- 2. typical-p, at temperature 1
    if (typical_p < 1.f) {
        const float m = view_max<REG>(c, red, use);
        if (m != -INFINITY) {
            const float sum = block_sum1(thread_sum<REG>(c, [&](int, int, unsigned h) { return takes_part(h) ? expf(h2f((uint16_t)h) - m) : 0.f; }), red, use);
            const float lse = m + logf(sum);
            r_lse = lse;
            float P[AD_SLOTS];                                 // REG: p_i, 0 where the entry takes no part
            int K[AD_SLOTS];                                   // REG: first s_i's bits, then the key of d_i
            float a[2];
            a[0] = thread_sum<REG>(c, [&](int slot, int, unsigned h) {
                const float s = lse - h2f((uint16_t)h);
                const float pr = takes_part(h) ? expf(-s) : 0.f;
                if constexpr (REG) { P[slot] = pr; K[slot] = __float_as_int(s); }
                return takes_part(h) ? pr * s : 0.f;
            });
            a[1] = thread_sum<REG>(c, [&](int slot, int, unsigned h) {
                if constexpr (REG) return P[slot];
                else return takes_part(h) ? expf(-(lse - h2f((uint16_t)h))) : 0.f;
            });
            block_sum<2>(a, red, use);
            const float H = a[0], mass_all = a[1];
            r_h = H;
            // the key of an entry: the bits of d_i = |s_i - H| (non-negative, so the bits order as the values do); none for an entry that takes no part
            auto key_of = [&](unsigned h) { return takes_part(h) ? __float_as_int(fabsf((lse - h2f((uint16_t)h)) - H)) : 0x7FFFFFFF; };
            int maxkey = 0;
            each<REG>(c, [&](int slot, int, unsigned h) {
                int k;
                if constexpr (REG) { k = takes_part(h) ? __float_as_int(fabsf(__int_as_float(K[slot]) - H)) : 0x7FFFFFFF; K[slot] = k; }
                else k = key_of(h);
                if (takes_part(h)) maxkey = max(maxkey, k);
            });
            maxkey = q4::block_max(maxkey, ired, use);
            int hi = maxkey;                                   // the mass of {key <= hi} reaches typical_p (or no set does: everything stays)
            if (mass_all >= typical_p) {
                int lo = -1;                                   // ... that of {key <= lo} does not
                while (hi - lo > 1) {
                    const int mid = lo + (hi - lo) / 2;
                    const float mass = block_sum1(thread_sum<REG>(c, [&](int slot, int, unsigned h) {
                        if constexpr (REG) return K[slot] <= mid ? P[slot] : 0.f;
                        else return key_of(h) <= mid ? expf(-(lse - h2f((uint16_t)h))) : 0.f;
                    }), red, use);
                    if (mass >= typical_p) hi = mid; else lo = mid;
                }
            }
            r_d = __int_as_float(hi);
            mask_pass<REG>(c, [&](int slot, int, unsigned h) {
                if constexpr (REG) return K[slot] <= hi;
                else return key_of(h) <= hi;
            });
        }
    }

    // ---- 3. Mirostat v2, at the sampler's temperature
    if (miro) {
        const float m = view_max<REG>(c, red, use);
        mu_p = s_mu;                                           // (behind view_max's barrier)
        float lse_kept = none;
        int valid = -1;
        if (m != -INFINITY) {
            const float mw = m / temp;
            const float sum = block_sum1(thread_sum<REG>(c, [&](int, int, unsigned h) { return takes_part(h) ? expf(h2f((uint16_t)h) / temp - mw) : 0.f; }), red, use);
            const float lse_t = mw + logf(sum);
            const float T_m = lse_t - mu_p * AD_LN2;
            r_lset = lse_t; r_tm = T_m;
            int arg = -1;                                      // the entry of largest w, lowest index: needed only where the threshold lies above it
            if (!(mw >= T_m)) {
                int first = -0x7FFFFFFF;
                each<REG>(c, [&](int, int i, unsigned h) { if (takes_part(h) && h2f((uint16_t)h) == m) first = max(first, -i); });
                arg = -q4::block_max(first, ired, use);
            }
            mask_pass<REG>(c, [&](int, int i, unsigned h) { return h2f((uint16_t)h) / temp >= T_m || i == arg; });
            // the side buffer: w of what stayed, -inf elsewhere, and their log-sum-exp (the pass that sums is the pass that stores)
            const float sumk = block_sum1(thread_sum<REG>(c, [&](int, int i, unsigned h) {
                const float w = h2f((uint16_t)h) / temp;
                side[i] = takes_part(h) ? w : -INFINITY;
                return takes_part(h) ? expf(w - mw) : 0.f;
            }), red, use);
            lse_kept = mw + logf(sumk);
            valid = p;
        }
        if (tid == 0) {
            mu_ring[p] = mu_p;
            side[n] = __int_as_float(valid);
            side[n + 1] = lse_kept;
        }
    }

    // ---- the record and what changed
    if (rec != nullptr) {                                      // (block-uniform)
        const float kept = block_sum1(thread_sum<REG>(c, [&](int, int, unsigned h) { return takes_part(h) ? 1.f : 0.f; }), red, use);
        if (tid == 0) {
            float* r = rec + (size_t)(rec_by_pos ? p : 0) * AD_REC;
            r[0] = r_ts; r[1] = r_h; r[2] = r_d; r[3] = mu_p; r[4] = r_tm; r[5] = __int_as_float((int)kept); r[6] = r_lse; r[7] = r_lset;
        }
    }
    if constexpr (REG) {
#pragma unroll
        for (int kq = 0; kq < AD_Q; kq++) {
            const int u = tid + kq * LB_T;
            if (u < c.n8 && (c.dirty >> kq & 1u)) c.lv[u] = c.pq[kq];
        }
    }
    if (c.tail < n && (c.dirty >> AD_Q & 1u)) logits[c.tail] = (q4_half)c.th;
}

// ---- host side: validation, the per-Sampler records, the stage's row ---------------------------------------------------------------------------------
const q4_adaptive_controls NEUTRAL = {1.f, 0.f, 0.f, 0.1f};

bool finite_f(float v) { return v == v && fabsf(v) != INFINITY; }
bool adaptive_valid(const q4_adaptive_controls* c) {
    return c->typical_p > 0.f && c->typical_p <= 1.f && finite_f(c->top_n_sigma) && c->top_n_sigma >= 0.f && finite_f(c->mirostat_tau) &&
           c->mirostat_tau >= 0.f && c->mirostat_eta > 0.f && c->mirostat_eta <= 1.f;
}
bool adaptive_off(const q4_adaptive_controls* c) { return c->typical_p == 1.f && c->top_n_sigma == 0.f && c->mirostat_tau == 0.f; }
void fill_params(AdaptiveParams* P, const q4_adaptive_controls* c, float temperature) {
    memset(P, 0, sizeof(*P));
    P->typical_p = c->typical_p; P->top_n_sigma = c->top_n_sigma; P->tau = c->mirostat_tau; P->eta = c->mirostat_eta; P->temperature = temperature;
}

// what q4_sampler_set_adaptive keeps beside a Sampler (sampler_side.h)
struct Adaptive : DeviceBlock<AdaptiveParams> {
    q4_adaptive_controls c = NEUTRAL;
    float temperature = -1.f;          // the sampler's temperature of the last upload
    bool on() const { return !adaptive_off(&c); }
};
SamplerSides<Adaptive>& sides() {
    static SamplerSides<Adaptive> r;
    return r;
}
DeviceBlock<AdaptiveParams> g_op;      // q4_adaptive_mask's own block

int launch(q4_half* logits, int n, const AdaptiveParams* dev, float* mu, float* side, float* rec, int rec_by_pos, int seq_len, const int* tokens,
           const int* pPos) {
    if (n <= LB_T * AD_Q * 8) Q4_LAUNCH(adaptive_kernel<true>, dim3(1), dim3(LB_T), 0, logits, n, dev, mu, side, rec, rec_by_pos, seq_len, tokens, pPos);
    else Q4_LAUNCH(adaptive_kernel<false>, dim3(1), dim3(LB_T), 0, logits, n, dev, mu, side, rec, rec_by_pos, seq_len, tokens, pPos);
    Q4_LAUNCH_CHECK();
    return Q4_OK;
}

// rows [first, first + count) of the mu ring and the record ring become the none marker (every byte 0xFF: a NaN)
int rings_to_none(const Model* m, int first, int count) {
    if (first < 0 || count < 0 || first + count > m->adaptive_len) return Q4_ERR_ARG;
    if (count == 0) return Q4_OK;
    Q4_HIP(hipMemsetAsync(m->adaptive_mu + first, 0xFF, (size_t)count * sizeof(float), g_stream));
    Q4_HIP(hipMemsetAsync(m->adaptive_rec + (size_t)first * AD_REC, 0xFF, (size_t)count * AD_REC * sizeof(float), g_stream));
    return Q4_OK;
}

// LogitStage::prepare: Mirostat against the sampler's temperature (m null: a RunState the library did not build -- no rings, no records, Mirostat is
// Q4_ERR_ARG), the model's rings on first use, then the block, which carries the temperature
int prepare(const Sampler* sampler, Model* m, const Config* p, const void** block) {
    Adaptive& r = sides().of(sampler);
    if (r.c.mirostat_tau > 0.f && (!(sampler->temperature > 0.f) || !m)) {
        snprintf(g_last_error, sizeof(g_last_error), "Mirostat needs a sampler temperature above 0 and a Transformer the library built");
        return Q4_ERR_ARG;
    }
    if (m && !m->adaptive_mu) {                                // the first step that needs them: kept until q4_free_transformer
        float* ring = nullptr;
        const size_t cells = (size_t)p->seq_len * (1 + AD_REC) + (size_t)p->vocab_size + 2;
        if (hipMalloc((void**)&ring, cells * sizeof(float)) != hipSuccess) { (void)hipGetLastError(); return Q4_ERR_ALLOC; }
        m->adaptive_mu = ring;
        m->adaptive_rec = ring + p->seq_len;
        m->adaptive_side = ring + (size_t)p->seq_len * (1 + AD_REC);
        m->adaptive_len = p->seq_len;
        Q4_HIP(hipMemsetAsync(ring, 0xFF, cells * sizeof(float), g_stream));       // none everywhere; side_pos -1
    }
    if (r.temperature != sampler->temperature) r.dirty = true;
    if (r.stale()) {
        fill_params(&r.host, &r.c, sampler->temperature);
        r.temperature = sampler->temperature;
    }
    Q4_TRY(r.upload());
    *block = r.dev;
    return Q4_OK;
}

bool stage_on(const Sampler* sampler, const Model*) { return sides().on(sampler); }
int launch_step(const void* block, const Model* m, const Config* p, RunState* s) {
    return launch(s->logits, p->vocab_size, (const AdaptiveParams*)block, m ? m->adaptive_mu : nullptr, m ? m->adaptive_side : nullptr,
                  m ? m->adaptive_rec : nullptr, 1, m ? m->adaptive_len : p->seq_len, &(s->shared_data->tokens[0]), s->pos);
}
const void* stage_block(const Sampler* sampler) { return sides().block(sampler); }
void stage_forget(const Sampler* sampler) { sides().forget(sampler); }

}  // namespace

// (no row form: Mirostat's side buffer belongs to a launch, not to a position)
LogitStage q4::adaptive_stage = {stage_on, prepare, launch_step, stage_block, stage_forget, nullptr};

namespace q4 {

int adaptive_clear_positions(const Model* m, int pos, int nsteps) { return m->adaptive_mu ? rings_to_none(m, pos, nsteps) : Q4_OK; }
int adaptive_clear_ring(const Model* m) { return m->adaptive_mu ? rings_to_none(m, 0, m->adaptive_len) : Q4_OK; }
// q4_shift_context (the stream has drained): mu and the records of [first, first + M) move down by D, entry new_pos - 1 receives old entry n_pos - 1,
// side_pos is rebased
int adaptive_shift(const Model* m, int vocab, int n_pos, int first, int M, int D) {
    if (!m->adaptive_mu) return Q4_OK;
    const int new_pos = n_pos - D;
    float last = 0.f;
    int side_pos = -1;
    Q4_HIP(hipMemcpy(&last, m->adaptive_mu + n_pos - 1, sizeof(float), hipMemcpyDeviceToHost));
    if (M > 0) {                                               // through the host: source and destination overlap whenever M > D
        std::vector<float> rows((size_t)M * (1 + AD_REC));
        Q4_HIP(hipMemcpy(rows.data(), m->adaptive_mu + first, (size_t)M * sizeof(float), hipMemcpyDeviceToHost));
        Q4_HIP(hipMemcpy(rows.data() + M, m->adaptive_rec + (size_t)first * AD_REC, (size_t)M * AD_REC * sizeof(float), hipMemcpyDeviceToHost));
        Q4_HIP(hipMemcpy(m->adaptive_mu + first - D, rows.data(), (size_t)M * sizeof(float), hipMemcpyHostToDevice));
        Q4_HIP(hipMemcpy(m->adaptive_rec + (size_t)(first - D) * AD_REC, rows.data() + M, (size_t)M * AD_REC * sizeof(float), hipMemcpyHostToDevice));
    }
    if (new_pos >= 1) Q4_HIP(hipMemcpy(m->adaptive_mu + new_pos - 1, &last, sizeof(float), hipMemcpyHostToDevice));
    Q4_HIP(hipMemcpy(&side_pos, m->adaptive_side + vocab, sizeof(int), hipMemcpyDeviceToHost));
    side_pos = side_pos >= D ? side_pos - D : -1;
    Q4_HIP(hipMemcpy(m->adaptive_side + vocab, &side_pos, sizeof(int), hipMemcpyHostToDevice));
    return Q4_OK;
}
// q4_free_transformer: the graphs that hold the rings are gone and the device has drained
void adaptive_release(Model* m) {
    if (m->adaptive_mu) (void)hipFree(m->adaptive_mu);
    m->adaptive_mu = m->adaptive_rec = m->adaptive_side = nullptr;
    m->adaptive_len = 0;
}

}  // namespace q4

extern "C" {

int q4_sampler_set_adaptive(Sampler* sampler, const q4_adaptive_controls* controls) {
    if (!sampler || (controls && !adaptive_valid(controls))) return Q4_ERR_ARG;
    if (!controls && !sides().find(sampler)) return Q4_OK;     // off, and never on
    Adaptive& r = sides().of(sampler);
    r.c = controls ? *controls : NEUTRAL;
    r.dirty = true;
    return Q4_OK;
}
int q4_sampler_get_adaptive(const Sampler* sampler, q4_adaptive_controls* out) {
    if (!sampler || !out) return Q4_ERR_ARG;
    const Adaptive* r = sides().find(sampler);
    *out = r ? r->c : NEUTRAL;
    return Q4_OK;
}

// "typical_p=0.9,top_n_sigma=1.5,mirostat_tau=5,mirostat_eta=0.1": any subset, any order, each key at most once; a key that is left out keeps its
// neutral value (mirostat_eta: 0.1). An unknown or repeated key, a key without a value, a number with trailing text, a trailing comma or a value the
// setter would refuse: Q4_ERR_ARG, *out untouched.
int q4_parse_adaptive(const char* text, q4_adaptive_controls* out) {
    if (!text || !out) return Q4_ERR_ARG;
    q4_adaptive_controls c = NEUTRAL;
    unsigned seen = 0u;
    const char* p = text;
    while (*p) {
        char key[OPTION_KEY_CAP], val[64];
        if (!next_option(&p, key, val, sizeof(val))) return Q4_ERR_ARG;
        const int which = !strcmp(key, "typical_p") ? 0 : !strcmp(key, "top_n_sigma") ? 1 : !strcmp(key, "mirostat_tau") ? 2 : !strcmp(key, "mirostat_eta") ? 3 : -1;
        if (which < 0 || (seen >> which & 1u)) return Q4_ERR_ARG;
        seen |= 1u << which;
        char* rest = nullptr;
        float* f = which == 0 ? &c.typical_p : which == 1 ? &c.top_n_sigma : which == 2 ? &c.mirostat_tau : &c.mirostat_eta;
        *f = strtof(val, &rest);
        if (*rest || rest == val) return Q4_ERR_ARG;
    }
    if (!adaptive_valid(&c)) return Q4_ERR_ARG;
    *out = c;
    return Q4_OK;
}

int q4_get_adaptive_records(const Transformer* t, int first_pos, int n, float* out) {
    const Model* m = t ? model_of(&t->state) : nullptr;
    if (!m || !m->adaptive_rec || !out || first_pos < 0 || n < 0 || (long long)first_pos + n > m->adaptive_len) return Q4_ERR_ARG;
    Q4_HIP(hipStreamSynchronize(g_stream));
    if (n > 0) Q4_HIP(hipMemcpy(out, m->adaptive_rec + (size_t)first_pos * AD_REC, (size_t)n * AD_REC * sizeof(float), hipMemcpyDeviceToHost));
    return Q4_OK;
}

int q4_adaptive_mask(q4_half* logits, int n, const q4_adaptive_controls* controls, float temperature, float* mu_ring, float* side, const int* tokens,
                     const int* pPos, float* record) {
    if (!logits || n < 1 || !controls || !adaptive_valid(controls)) return Q4_ERR_ARG;
    if (controls->mirostat_tau > 0.f && (!(temperature > 0.f) || !finite_f(temperature) || !mu_ring || !side || !tokens || !pPos)) return Q4_ERR_ARG;
    if (adaptive_off(controls)) return Q4_OK;
    fill_params(&g_op.host, controls, temperature);
    g_op.dirty = true;
    Q4_TRY(g_op.upload());
    const bool miro = controls->mirostat_tau > 0.f;
    return launch(logits, n, g_op.dev, miro ? mu_ring : nullptr, miro ? side : nullptr, record, 0, Q4_MAX_SEQ_LEN, miro ? tokens : nullptr,
                  miro ? pPos : nullptr);
}

}  // extern "C"
