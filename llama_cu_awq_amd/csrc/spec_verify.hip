// spec_verify.hip -- the verify pass of speculative greedy decoding (spec_verify.h): an embedding launch (row 0 from the ring, rows
// 1 .. D from the drafts in the kernel argument), the prompt pass's layer loop, the classifier for all rows on one read of wcls, the accept launch.
// With log-probability records on (q4_set_pass_logprobs): the row form of the record launch behind the classifier (run_verify_pass).
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <math.h>
#include "gemv_q4.h"
#include "spec_verify.h"

namespace q4 {

// ---- classifier: final rmsnorm + fp16 GEMV for n residual rows --------------------------------------------------------------------------------------
// One sixteen-wave block per CU owns a contiguous range of vocabulary rows (cls_strip_kernel's split: d / CUs rows, the first d % CUs blocks one more). The
// block normalises the n rows of x once into LDS (rmsnorm_kernel's arithmetic: sumsq8 chunk partials, rms_scale_from_partials, rms_apply8; two rows per
// round, one per half of the block); then a wave takes two vocabulary rows at a time into registers (2 x 8 pieces of 1 KiB, non-temporal) and multiplies
// them with every row of x, read from LDS once per pair. Per lane and output: for slots s = 0 .. 7: acc = four v_dot2c from zero, sum += acc; then
// wave_sum and one rounding -- gemv_f16_kernel's and cls_strip_kernel's arithmetic (gemv_strip_cls.h), so a row's logits are the bits either writes for
// that row alone. x in LDS and not in registers: eight rows of 32 VGPRs do not fit beside the weights; two weight rows per read of x halve the LDS
// traffic (n x 8 KiB of LDS reads per 16 KiB of weights: at n = 8 four times the HBM stream's bytes, under a third of the LDS's rate).
// NC: 8-half chunks of a row -- 512 (dim 4096) or 640 (dim 5120, q4_set_pass_13b: ten pieces per row, gemv_f16_kernel's and cls_strip_kernel<10>'s
// chain; the block normalises one row per round with its first ten waves, the canonical sum over 640 partials).
constexpr int VC_WAVES = 16;
static size_t verify_cls_lds(int n, int nc) { return (size_t)n * nc * 16 + 2 * (size_t)nc * 4; }

template <int NC>
__global__ void __launch_bounds__(VC_WAVES * 64) verify_cls_kernel(const u32x4* __restrict__ x, const u32x4* __restrict__ rms_w, const u32x4* __restrict__ wcls,
                                                                    q4_half* __restrict__ out, const int n, const int dim, const int d, const unsigned rbase,
                                                                    const unsigned rrem) {
    constexpr int VC_CHUNKS = NC, VC_NS = NC / 64;
    constexpr bool TWO = 2 * NC == VC_WAVES * 64;                                     // two rows per round, one per half of the block; else one, on the first NC threads
    static_assert(NC % 64 == 0 && NC <= VC_WAVES * 64 && (TWO || 2 * NC > VC_WAVES * 64), "chunks of a row against the block");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    u32x4* xn = reinterpret_cast<u32x4*>(smem);                                       // [n][VC_CHUNKS]: chunk j = s * 64 + lane of row t
    float* part = reinterpret_cast<float*>(smem + (size_t)n * VC_CHUNKS * 16);        // [2][VC_CHUNKS]
    const unsigned tid = threadIdx.x, lane = tid & 63u;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const unsigned r0 = blockIdx.x * rbase + (blockIdx.x < rrem ? blockIdx.x : rrem);
    const int nr = (int)(rbase + (blockIdx.x < rrem ? 1u : 0u));
    if (nr == 0) return;                                                              // (the whole block)

    const unsigned c = TWO ? tid & (VC_CHUNKS - 1) : (tid < (unsigned)VC_CHUNKS ? tid : (unsigned)VC_CHUNKS - 1u);
    const int half = TWO ? wave >> 3 : 0;
    const bool stager = TWO || tid < (unsigned)VC_CHUNKS;                             // (wave-uniform: NC is whole waves)
    const u32x4 wraw = rms_w[c];
    for (int t0 = 0; t0 < n; t0 += TWO ? 2 : 1) {
        const int t = t0 + half;
        const bool act = stager && t < n;                                             // (wave-uniform)
        u32x4 xraw = {0u, 0u, 0u, 0u};
        if (act) xraw = x[(size_t)t * VC_CHUNKS + c];
        if (stager) part[half * VC_CHUNKS + c] = sumsq8(xraw, 0.f);
        __syncthreads();
        if (act) xn[t * VC_CHUNKS + c] = rms_apply8(xraw, wraw, rms_scale_from_partials<VC_CHUNKS>(part + half * VC_CHUNKS, VC_CHUNKS, dim));
        __syncthreads();
    }

    const int rend = (int)r0 + nr;
    for (int r = (int)r0 + 2 * wave; r < rend; r += 2 * VC_WAVES) {
        const int rb = r + 1 < rend ? r + 1 : r;                                      // an odd range's last pair: the same row twice, stored once
        u32x4 W[2][VC_NS];
#pragma unroll
        for (int s = 0; s < VC_NS; s++) {
            W[0][s] = ld_nt(wcls + (size_t)r * VC_CHUNKS + s * 64 + lane);
            W[1][s] = ld_nt(wcls + (size_t)rb * VC_CHUNKS + s * 64 + lane);
        }
        for (int t = 0; t < n; t++) {
            float sum0 = 0.f, sum1 = 0.f;
#pragma unroll
            for (int s = 0; s < VC_NS; s++) {
                const u32x4 X = xn[t * VC_CHUNKS + s * 64 + lane];
                float acc0 = 0.f, acc1 = 0.f;
#pragma unroll
                for (int e = 0; e < 4; e++) {
                    acc0 = __builtin_amdgcn_fdot2(as_h2(W[0][s][e]), as_h2(X[e]), acc0, false);
                    acc1 = __builtin_amdgcn_fdot2(as_h2(W[1][s][e]), as_h2(X[e]), acc1, false);
                }
                sum0 += acc0;
                sum1 += acc1;
            }
            float v0 = wave_sum(sum0), v1 = wave_sum(sum1);
            v0 *= 1.0f;                                                               // alpha, gpu_kernels.h:135
            v1 *= 1.0f;
            if (lane == 0) {
                out[(size_t)t * d + r] = f2h(v0);
                if (rb != r) out[(size_t)t * d + rb] = f2h(v1);
            }
        }
    }
}

bool verify_cls_covers(int dim, int vocab) { return (dim == 4096 || dim == 5120) && vocab >= 8 && (vocab & 7) == 0; }

template <int NC>
static int launch_verify_cls_nc(q4_half* logits, const q4_half* x, const q4_half* rms_w, const q4_half* wcls, int dim, int vocab, int n) {
    Q4_TRY(lds_opt_in((const void*)verify_cls_kernel<NC>, verify_cls_lds(PROMPT_PASS_MAX, NC)));
    const unsigned nb = (unsigned)cu_count();
    Q4_LAUNCH(verify_cls_kernel<NC>, dim3(nb), dim3(VC_WAVES * 64), verify_cls_lds(n, NC), reinterpret_cast<const u32x4*>(x), reinterpret_cast<const u32x4*>(rms_w),
              reinterpret_cast<const u32x4*>(wcls), logits, n, dim, vocab, (unsigned)vocab / nb, (unsigned)vocab % nb);
    Q4_LAUNCH_CHECK();
    return Q4_OK;
}
int launch_verify_cls(q4_half* logits, const q4_half* x, const q4_half* rms_w, const q4_half* wcls, int dim, int vocab, int n) {
    if (!verify_cls_covers(dim, vocab) || n < 1 || n > PROMPT_PASS_MAX) return Q4_ERR_UNSUPPORTED_SIZE;
    return dim == 4096 ? launch_verify_cls_nc<512>(logits, x, rms_w, wcls, dim, vocab, n) : launch_verify_cls_nc<640>(logits, x, rms_w, wcls, dim, vocab, n);
}

// ---- accept -----------------------------------------------------------------------------------------------------------------------------------------
// One block. Row by row argmax_kernel's rule (q4_kernels.hip): 16-byte loads, the first maximum inside a thread, the tail past the last whole chunk, value
// then lower index across threads, 0 for a row without a finite or +inf entry. Then m = the leading drafts the rows confirm, the copies of row m, and --
// in argmax_kernel's order -- the ring entries, a fence, both position words. No atomics; one writer per word.
// GIVEN (a pass under the sampler): the rows' tokens are win[0 .. d.n], what the row form of the sampler left (q4_sampling.hip), and no row is searched;
// the rows then hold probabilities, which is what a sampled step leaves in RunState::logits. Everything behind the tokens is the one code.
template <bool GIVEN>
__global__ void __launch_bounds__(1024) verify_accept_kernel(const q4_half* logits, const int ld, const int size, const VerifyDrafts d, const q4_half* x, const int dim,
                                                             q4_half* logits_out, q4_half* x_out, int* ring, volatile int* pPos, int* pPosGpu, int* report,
                                                             const int* win) {
    __shared__ float sval[16];
    __shared__ int sidx[16];
    __shared__ int s_win[PROMPT_PASS_MAX];
    __shared__ int s_m;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n8 = size >> 3;
    if (GIVEN) {
        if (tid <= d.n) s_win[tid] = win[tid];
        __syncthreads();
    }
    for (int t = 0; !GIVEN && t <= d.n; t++) {
        const q4_half* row = logits + (size_t)t * ld;
        float max_val = -INFINITY;
        int max_pos = 0x7fffffff;
        for (int u = tid; u < n8; u += blockDim.x) {
            const u32x4 v = reinterpret_cast<const u32x4*>(row)[u];
#pragma unroll
            for (int e = 0; e < 4; e++) {
                const h2 p = as_h2(v[e]);
                const float a = (float)p.x, b = (float)p.y;
                if (a > max_val) { max_val = a; max_pos = u * 8 + 2 * e; }
                if (b > max_val) { max_val = b; max_pos = u * 8 + 2 * e + 1; }
            }
        }
        for (int i = n8 * 8 + tid; i < size; i += blockDim.x) {
            const float v = h2f(row[i]);
            if (v > max_val) { max_val = v; max_pos = i; }
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const float ov = __shfl_xor(max_val, off);
            const int op = __shfl_xor(max_pos, off);
            if (ov > max_val || (ov == max_val && op < max_pos)) { max_val = ov; max_pos = op; }
        }
        if (lane == 0) { sval[wave] = max_val; sidx[wave] = max_pos; }
        __syncthreads();
        if (tid == 0) {
            const int nw = blockDim.x >> 6;
            for (int w = 1; w < nw; w++)
                if (sval[w] > max_val || (sval[w] == max_val && sidx[w] < max_pos)) { max_val = sval[w]; max_pos = sidx[w]; }
            if (max_pos == 0x7fffffff) max_pos = 0;          // all NaN / -inf
            s_win[t] = max_pos;
        }
        __syncthreads();                                     // sval / sidx are free for the next row
    }
    if (tid == 0) {
        int m = 0;
        while (m < d.n && s_win[m] == d.tok[m]) m++;
        s_m = m;
    }
    __syncthreads();
    const int m = s_m;
    {   // what step p + m leaves: its logits and its residual stream
        const q4_half* lrow = logits + (size_t)m * ld;
        for (int u = tid; u < n8; u += blockDim.x) reinterpret_cast<u32x4*>(logits_out)[u] = reinterpret_cast<const u32x4*>(lrow)[u];
        for (int i = n8 * 8 + tid; i < size; i += blockDim.x) logits_out[i] = lrow[i];
        if (x_out != nullptr)
            for (int u = tid; u < (dim >> 3); u += blockDim.x) reinterpret_cast<u32x4*>(x_out)[u] = reinterpret_cast<const u32x4*>(x + (size_t)m * dim)[u];
    }
    __threadfence();
    __syncthreads();
    if (tid == 0) {
        const int p = *pPosGpu;
        for (int i = 0; i <= m; i++) ring[p + 1 + i] = s_win[i];
        if (report != nullptr) {
            for (int i = 0; i < PROMPT_PASS_MAX; i++) report[i] = i <= d.n ? s_win[i] : -1;
            report[PROMPT_PASS_MAX] = m;
        }
        __threadfence_system();                              // the host may be spinning on *pPos (q4_wait_pos)
        *pPos = p + m + 1;
        *pPosGpu = p + m + 1;
    }
}

int launch_verify_accept(const q4_half* logits, int ld, int size, const VerifyDrafts& d, const int* win, const q4_half* x, int dim, q4_half* logits_out,
                         q4_half* x_out, int* ring, volatile int* pPos, int* pPosGpu, int* report) {
    if (d.n < 1 || d.n > VERIFY_MAX_DRAFT || size < 1 || ld < size || (ld & 7) || (dim & 7) || !logits || !logits_out || !ring || !pPos || !pPosGpu) return Q4_ERR_ARG;
    if (win) Q4_LAUNCH(verify_accept_kernel<true>, dim3(1), dim3(1024), 0, logits, ld, size, d, x, dim, logits_out, x ? x_out : nullptr, ring, pPos, pPosGpu, report, win);
    else Q4_LAUNCH(verify_accept_kernel<false>, dim3(1), dim3(1024), 0, logits, ld, size, d, x, dim, logits_out, x ? x_out : nullptr, ring, pPos, pPosGpu, report, win);
    Q4_LAUNCH_CHECK();
    return Q4_OK;
}
int verify_drafts(const int* draft, int n_draft, int vocab, VerifyDrafts* out) {
    if (!draft || n_draft < 1 || n_draft > VERIFY_MAX_DRAFT) return Q4_ERR_ARG;
    *out = VerifyDrafts{n_draft, {}};
    for (int i = 0; i < n_draft; i++) {
        if (vocab >= 0 && (draft[i] < 0 || draft[i] >= vocab)) return Q4_ERR_ARG;
        out->tok[i] = draft[i];
    }
    return Q4_OK;
}

// ---- the pass ---------------------------------------------------------------------------------------------------------------------------------------
// the n rows' embeddings and positions (prompt_embed_kernel with rows 1 .. D taken from the argument)
__global__ void verify_embed_kernel(q4_half* xs, const q4_half* table, int dim, const int* tokens, const VerifyDrafts d, const int* pPos, int* pos_arr) {
    const int u = blockIdx.x * blockDim.x + threadIdx.x, t = blockIdx.y;
    const int pos = *pPos + t;
    if (u == 0) pos_arr[t] = pos;
    if (u >= (dim >> 3)) return;
    const int token = t == 0 ? tokens[pos] : d.tok[t - 1];
    reinterpret_cast<u32x4*>(xs + (size_t)t * dim)[u] = reinterpret_cast<const u32x4*>(table + (size_t)token * dim)[u];
}

// The draft view (spec_verify.h): view[lo .. p] from the ring, view[p + 1 .. p + d.n] from the argument, p = *pPos, lo = max(0, p + 1 - window). A grid of
// divUp(window + PROMPT_PASS_MAX, 256) blocks covers it; nothing outside [0, len) is touched.
__global__ void verify_view_kernel(int* view, int len, const int* tokens, const VerifyDrafts d, const int* pPos, int window) {
    const int p = *pPos;
    const int lo = p + 1 - window > 0 ? p + 1 - window : 0;
    const int i = lo + (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (p < 0 || i > p + d.n || i >= len) return;
    view[i] = i <= p ? tokens[i] : d.tok[i - p - 1];
}

int run_verify_pass(const Config* p, RunState* s, const TransformerWeights* w, Model* m, int pos0, const int* draft, int n_draft, Sampler* sampler,
                    const float* coins, const Sampler* stages) {
    if (sampler && (!coins || sampler->vocab_size != p->vocab_size)) return Q4_ERR_ARG;
    if (sampler) Q4_TRY(sample_rows_prepare(sampler));       // (scratch on first use and the LDS opt-in: in front of the pass's first launch)
    if (!prompt_pass_covers(p, m) || !verify_cls_covers(p->dim, p->vocab_size)) return Q4_ERR_ARG;
    VerifyDrafts d;
    Q4_TRY(verify_drafts(draft, n_draft, p->vocab_size, &d));
    const int dim = p->dim, n = n_draft + 1;
    Q4_TRY(prompt_pass_rows(m, p));
    const PassScratch& rows = m->pass;
    const bool records = m->logprobs_k >= 0;                 // (admitted with records on: q4_set_pass_logprobs, q4_passes.hip)
    if (records && !m->pass_logprobs) return Q4_ERR_ARG;
    Q4_TRY(pass_logit_rows(m, p));                           // (behind the rows: the PROMPT_PASS_MAX tokens the row form of the sampler leaves for the accept launch)
    if (records && sampler) Q4_TRY(pass_side_rows(m, p));
    const bool staged = m->pass_stages && any_stage_on(stages, m);      // (admitted: q4_set_pass_stages, every stage that is on has a row form, no records)
    if (staged && (records || !stages_take_rows(stages, m) || pos0 + n_draft >= p->seq_len)) return Q4_ERR_ARG;
    if (staged) Q4_TRY(pass_draft_view(m, p));
    Q4_LAUNCH(verify_embed_kernel, dim3(divUp(dim >> 3, 256), n), dim3(256), 0, rows.x, w->token_embedding_table, dim, (const int*)s->shared_data->tokens, d,
              (const int*)s->pos, rows.pos);
    Q4_LAUNCH_CHECK();
    Q4_TRY(prompt_pass_layers(p, s, w, m, pos0, n));
    Q4_TRY(launch_verify_cls(rows.logit_rows, rows.x, w->rms_final_weight, w->wcls, dim, p->vocab_size, n));
    // Records p .. p + D, in front of the accept launch (it advances the position): a greedy row's token_logprob is entry 0; under the sampler the raw rows go
    // aside in front of the sampler's row form, which normalises them in place, and the rows' tokens are looked up behind it -- the order of the sampled step
    if (records) Q4_TRY(launch_logprobs_rows(m, p, s, rows.logit_rows, p->vocab_size, n, sampler ? LP_SAMPLED : LP_GREEDY));
    // The logit stages that are on, in table order, each row at its own position; in front of them the draft view their row forms read in place of the ring
    if (staged) {
        Q4_LAUNCH(verify_view_kernel, dim3(divUp(Q4_MAX_DRY_WINDOW + PROMPT_PASS_MAX, 256)), dim3(256), 0, rows.view, p->seq_len, (const int*)s->shared_data->tokens, d,
                  (const int*)s->pos, (int)Q4_MAX_DRY_WINDOW);
        Q4_LAUNCH_CHECK();
        Q4_TRY(launch_stage_rows(stages, m, p, rows.logit_rows, p->vocab_size, n, rows.view, rows.pos));
    }
    int* win = nullptr;
    if (sampler) {      // each row sampled in place with its own position's coin, as the step at that position would; then the accept on those tokens
        win = reinterpret_cast<int*>(rows.logit_rows + (size_t)PROMPT_PASS_MAX * p->vocab_size);
        Q4_TRY(launch_sample_rows(sampler, rows.logit_rows, p->vocab_size, n, coins, s->pos, win));
        if (records) Q4_TRY(launch_logprobs_pick_rows(m, p, s, n, win));
    }
    return launch_verify_accept(rows.logit_rows, p->vocab_size, p->vocab_size, d, win, rows.x, dim, s->logits, s->x, (int*)s->shared_data->tokens, &(s->shared_data->pos),
                                s->pos, nullptr);
}

}  // namespace q4

using namespace q4;

// Op-level forms of the two launches, for tests and tools (include/llama2_q4.h)
extern "C" {

int q4_verify_classifier(q4_half* logits, const q4_half* x, const q4_half* rms_w, const q4_half* wcls, int dim, int vocab, int n_rows) {
    if (!logits || !x || !rms_w || !wcls || n_rows < 1 || n_rows > PROMPT_PASS_MAX) return Q4_ERR_ARG;
    return launch_verify_cls(logits, x, rms_w, wcls, dim, vocab, n_rows);
}

int q4_verify_accept(const q4_half* logits, int ld, int size, const int* draft, int n_draft, const q4_half* x, int dim, q4_half* logits_out, q4_half* x_out,
                     int* ring, int* pos_host, int* pos_dev, int* report) {
    VerifyDrafts d;
    Q4_TRY(verify_drafts(draft, n_draft, -1, &d));
    return launch_verify_accept(logits, ld, size, d, nullptr, x, dim, logits_out, x_out, ring, pos_host, pos_dev, report);
}

int q4_verify_accept_tokens(const q4_half* logits, int ld, int size, const int* draft, int n_draft, const int* tokens_dev, const q4_half* x, int dim,
                            q4_half* logits_out, q4_half* x_out, int* ring, int* pos_host, int* pos_dev, int* report) {
    VerifyDrafts d;
    if (!tokens_dev) return Q4_ERR_ARG;
    Q4_TRY(verify_drafts(draft, n_draft, -1, &d));
    return launch_verify_accept(logits, ld, size, d, tokens_dev, x, dim, logits_out, x_out, ring, pos_host, pos_dev, report);
}

}  // extern "C"
