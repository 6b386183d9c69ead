// prompt_pass_kv8.hip -- the launches a prompt or verify pass adds for a model with the FP8 (e4m3) K / V cache (prompt_pass_kv8.h; q4_set_pass_kv8,
// DESIGN.md section 3.7 "FP8 cache"). Not in the reference.
//
// APPEND, THEN ATTEND. The step's attention launch quantises the position's staging row in registers, computes with the round-tripped bytes -- for the
// current row too -- and appends them. A pass splits that in two launches: pass_kv8_append_kernel runs the same kv8_quantise on every token's staging
// row and stores bytes and exponents as kv8_append does; the attention launch behind it then reads rows [0, pos[t]] from the cache, where row pos[t]
// holds exactly the bytes and the exponent the step had in registers. So every score and every P . V term is the step's, and because the append is a
// launch of its own no attention block runs beside a writer of the rows it reads.
// Head size 128 only (LPR = 8): the one the admitted shapes have (prompt_pass_covers).
#include <hip/hip_runtime.h>
#include <math.h>
#include "attention_kv8.h"
#include "prompt_pass.h"
#include "prompt_pass_kv8.h"

namespace q4 {

constexpr int PK8_LPR = 8;                                   // lanes per cache row of a 128-wide head
constexpr int PK8_HS = PK8_LPR * 16;

// One wave per (token, kv head): its eight row groups all hold the head's staging row (kv8_quantise's layout), the first stores
__global__ void __launch_bounds__(64) pass_kv8_append_kernel(const PassKv8 c, const q4_half* k_rows, const q4_half* v_rows) {
    const int t = blockIdx.x, kvh = blockIdx.y;
    const unsigned tid = threadIdx.x;
    const int sub = tid % PK8_LPR;
    const size_t hoff = (size_t)kvh * PK8_HS + sub * 16;
    const int pos = __builtin_amdgcn_readfirstlane(c.pos[t]);
    u32x4 kq, vq;
    int ke, ve;
    kv8_quantise<PK8_LPR>(k_rows + (size_t)t * c.kv_dim + hoff, kq, ke);
    kv8_quantise<PK8_LPR>(v_rows + (size_t)t * c.kv_dim + hoff, vq, ve);
    Kv8Args a = {};
    a.k8 = c.k8; a.v8 = c.v8; a.k_exp = c.k_exp; a.v_exp = c.v_exp; a.kv_dim = c.kv_dim; a.exp_stride = c.exp_stride;
    kv8_append<PK8_LPR>(a, kvh, pos, tid, hoff, kq, ke, vq, ve);
}

// The one-pass form is attention_kv8_kernel<LPR, U, NW, ROW = true> (attention_kv8.h): block (t, h) is the step's block h at position pos[t] with the row
// already in the cache; its resource ends at pos[t] + 1 rows, so later tokens' rows never reach it.

// The split-context form: block (h, sp) is attention_kv8_split_kernel's block of chunk sp, once for all tokens of the pass. It requests the chunk's K
// bytes, V bytes and exponents ONCE -- the step's request order, the resource bounded at the LAST token's size -- and loops over the tokens: each
// token's record is the step's middle restated on the same helpers (kv8_dot16, row_sum, round_h, wave_max / row16_max, expf, kv8_axpy16 over u in order,
// wave_sum / row16_sum, kv8_store_partial, split_store_record<false, NW>) with size = pos[t] + 1, written to the token's own record area as plain
// floats; prompt_merge_kernel merges them. No tag, no counter, no atomic.
//  * MASKED LANES. The step bounds its resource at its own position, so a row at or above it arrives as zero bytes with exponent 0. Here a row in
//    (pos[t], pos[last]] holds a later token's bytes: such a lane SELECTS zero bytes and exponent 0 -- it does not multiply what it loaded by a zero
//    probability (an e4m3fn byte 0x7F is NaN, and 0 * NaN is not 0) -- and its score is -inf, as the step's.
//  * LDS across tokens: as prompt_split_attention_kernel -- token t + 1 writes red_max in front of its first barrier and outp / red_sum behind it, and
//    every reader of token t's has issued its reads before it arrives at that barrier.
struct PassKv8Split {
    PassKv8 c;
    float* records;
    const q4_half* q;
    size_t tok_stride;
    int dim, nsp;
    float alpha;
};
template <int U>
__global__ void __launch_bounds__(ATT_NW * 64) pass_kv8_split_kernel(const PassKv8Split a) {
    constexpr int LPR = PK8_LPR, NW = ATT_NW, R = 64 / LPR, stride = NW * R, CHUNK = stride * U, HS = PK8_HS;
    static_assert(NW == 16, "the reductions read sixteen entries");
    __shared__ __attribute__((aligned(16))) float lds[32 + NW * HS];
    float* red_max = lds;
    float* red_sum = lds + 16;
    float* outp = lds + 32;                                  // [NW][HS]
    const unsigned tid = threadIdx.x, lane = tid & 63u;
    const int wave = tid >> 6, row = lane / LPR, sub = lane % LPR;
    const int h = blockIdx.x, sp = blockIdx.y, kvh = h / a.c.kv_mul;
    const int ntok = a.c.ntok, kv_dim = a.c.kv_dim;
    const int rec = HS + ATT_REC_PAD;
    const int t_base = sp * CHUNK;
    const size_t hoff = (size_t)kvh * HS + sub * 16;
    const int size_last = __builtin_amdgcn_readfirstlane(a.c.pos[ntok - 1]) + 1;      // rows the pass may read: [0, size_last)
    auto neutral = [&](int t) {      // a chunk wholly above pos[t]: the step's neutral record (m = -inf, l = 0)
        const f32x4 r4 = {-INFINITY, 0.f, 0.f, 0.f};
        *reinterpret_cast<f32x4*>(a.records + (size_t)t * a.tok_stride + ((size_t)h * a.nsp + sp) * rec + HS) = r4;
    };
    if (t_base >= size_last) {
        if ((int)tid < ntok) neutral((int)tid);
        return;
    }
    const __amdgpu_buffer_rsrc_t rk = __builtin_amdgcn_make_buffer_rsrc((void*)a.c.k8, 0, (unsigned)size_last * (unsigned)kv_dim, 0x00020000);
    const __amdgpu_buffer_rsrc_t rv = __builtin_amdgcn_make_buffer_rsrc((void*)a.c.v8, 0, (unsigned)size_last * (unsigned)kv_dim, 0x00020000);
    const int8_t* kex = a.c.k_exp + (size_t)kvh * a.c.exp_stride;
    const int8_t* vex = a.c.v_exp + (size_t)kvh * a.c.exp_stride;
    u32x4 kb[U], vb[U];
    int ek[U], ev[U];
#pragma unroll
    for (int u = 0; u < U; u++)
        kb[u] = __builtin_amdgcn_raw_buffer_load_b128(rk, (unsigned)(t_base + wave * R + row + u * stride) * (unsigned)kv_dim + (unsigned)hoff, 0, 0);
#pragma unroll
    for (int u = 0; u < U; u++)
        vb[u] = __builtin_amdgcn_raw_buffer_load_b128(rv, (unsigned)(t_base + wave * R + row + u * stride) * (unsigned)kv_dim + (unsigned)hoff, 0, 0);
#pragma unroll
    for (int u = 0; u < U; u++) {
        const int r = t_base + wave * R + row + u * stride;
        ek[u] = r < size_last ? (int)kex[r] : 0;
        ev[u] = r < size_last ? (int)vex[r] : 0;
    }
    SplitArgs sa = {};
    sa.head_size = HS;
    const u32x4 zero = {0u, 0u, 0u, 0u};
    for (int t = 0; t < ntok; t++) {
        const int size = __builtin_amdgcn_readfirstlane(a.c.pos[t]) + 1;
        if (t_base >= size) {                                // (block-uniform: no barrier is skipped by part of the block)
            if (tid == 0) neutral(t);
            continue;
        }
        const q4_half* qh = a.q + (size_t)t * a.dim + (size_t)h * HS + sub * 16;
        const u32x4 q0 = *reinterpret_cast<const u32x4*>(qh);
        const u32x4 q1 = *reinterpret_cast<const u32x4*>(qh + 8);
        float scv[U];
        float wmax = -INFINITY;
#pragma unroll
        for (int u = 0; u < U; u++) {
            const bool live = t_base + wave * R + row + u * stride < size;
            float s = row_sum<LPR>(kv8_dot16(live ? kb[u] : zero, q0, q1));
            s = round_h(s * kv8_pow2(live ? ek[u] : 0) * a.alpha);
            scv[u] = live ? s : -INFINITY;
            wmax = fmaxf(wmax, scv[u]);
        }
        wmax = wave_max(wmax);
        if (lane == 0) red_max[wave] = wmax;
        __syncthreads();
        const float m = row16_max(red_max[lane & 15]);
        float acc[16];
#pragma unroll
        for (int e = 0; e < 16; e++) acc[e] = 0.f;
        float lsum = 0.f;
#pragma unroll
        for (int u = 0; u < U; u++) {
            const bool live = t_base + wave * R + row + u * stride < size;
            const float p = expf(scv[u] - m);                // fp32 probabilities here, 0 for masked positions
            if (sub == 0) lsum += p;
            kv8_axpy16(acc, live ? vb[u] : zero, p * kv8_pow2(live ? ev[u] : 0));
        }
        lsum = wave_sum(lsum);
        if (lane == 0) red_sum[wave] = lsum;
        kv8_store_partial<LPR>(acc, outp + wave * HS, lane, sub);
        __syncthreads();
        const float l = row16_sum(red_sum[lane & 15]);
        sa.partials = a.records + (size_t)t * a.tok_stride;
        split_store_record<false, NW>(sa, Handoff{}, outp, m, l, h, sp, a.nsp);
    }
}

// ---- host ------------------------------------------------------------------------------------------
static bool pass_kv8_ok(const PassKv8& c) {
    return c.k8 && c.v8 && c.k_exp && c.v_exp && c.pos && c.head_size == PK8_HS && c.kv_mul >= 1 && c.n_heads >= 1 && c.n_heads % c.kv_mul == 0 &&
           c.kv_dim == c.n_heads / c.kv_mul * PK8_HS && c.exp_stride >= 1 && c.ntok >= 1 && c.ntok <= PROMPT_PASS_MAX;
}

int launch_pass_kv8_append(const PassKv8& c, const q4_half* k_rows, const q4_half* v_rows) {
    if (!pass_kv8_ok(c) || !k_rows || !v_rows) return Q4_ERR_ARG;
    Q4_LAUNCH(pass_kv8_append_kernel, dim3((unsigned)c.ntok, (unsigned)(c.n_heads / c.kv_mul)), dim3(64), 0, c, k_rows, v_rows);
    Q4_LAUNCH_CHECK();
    return Q4_OK;
}

int launch_pass_kv8_attention(const PassKv8& c, q4_half* xb, const q4_half* q, int dim, float alpha) {
    if (!pass_kv8_ok(c) || !xb || !q || dim != c.n_heads * PK8_HS) return Q4_ERR_ARG;
    constexpr int SCORES = PASS_CONTEXT_MIN;                 // the form's bins end at 256 (pass_attention_plan)
    const size_t smem = (size_t)(32 + ATT_NW * PK8_HS + SCORES) * 4;
    const Kv8Args a = {xb, q, c.k8, c.v8, c.k_exp, c.v_exp, nullptr, nullptr, PK8_HS, c.kv_mul, c.kv_dim, c.exp_stride, c.pos, alpha, SCORES, nullptr, nullptr};
    Q4_LAUNCH((attention_kv8_kernel<PK8_LPR, 4, ATT_NW, true>), dim3((unsigned)(c.ntok * c.n_heads)), dim3(ATT_NW * 64), smem, a);
    Q4_LAUNCH_CHECK();
    return Q4_OK;
}

int launch_pass_kv8_split(const PassKv8& c, float* records, size_t tok_stride, const q4_half* q, int dim, float alpha, int chunk, int nsp) {
    if (!pass_kv8_ok(c) || !records || !q || dim != c.n_heads * PK8_HS || nsp < 1 || (chunk != 128 && chunk != 256) ||
        tok_stride < (size_t)c.n_heads * nsp * (PK8_HS + ATT_REC_PAD))
        return Q4_ERR_ARG;
    const PassKv8Split a = {c, records, q, tok_stride, dim, nsp, alpha};
    const dim3 grid((unsigned)c.n_heads, (unsigned)nsp);
    if (chunk == 128) Q4_LAUNCH(pass_kv8_split_kernel<1>, grid, dim3(ATT_NW * 64), 0, a);      // 16 waves x 8 rows
    else Q4_LAUNCH(pass_kv8_split_kernel<2>, grid, dim3(ATT_NW * 64), 0, a);
    Q4_LAUNCH_CHECK();
    return Q4_OK;
}

}  // namespace q4
