// cls_screen.hip -- the greedy step's classifier as an int8 screen and an exact refinement of the candidate rows (cls_screen.h: the method, the bound and
// the derivation of gamma), the kernel that builds a model's screening copy, and the op-level entry point of the tests.
#include <hip/hip_runtime.h>
#include <math.h>
#include <vector>
#include "q4_model.h"
#include "gemv_q4.h"
#include "lds_dma.h"

namespace q4 {

int g_greedy_screen = 1;
constexpr int STRIP_WAVES = 16, CLS_D = 4;   // gemv_strip_cls.h's block and ring depth (its launchers stay in q4_kernels.hip: the header is not included here)

// ---------------------------------------------------------------------------------------------------
// build: one wave per row. Pass 1 the row's largest magnitude, pass 2 (the row comes back out of L2) the bytes and the three sums in float64.
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    return v;
}
__global__ void __launch_bounds__(256) cls_screen_build_kernel(const q4_half* __restrict__ w, unsigned char* __restrict__ q8, float* __restrict__ scale,
                                                               float* __restrict__ ew, const int n, const int d) {
    const unsigned lane = threadIdx.x & 63u;
    const int row = (int)(blockIdx.x * 4u + (threadIdx.x >> 6));
    if (row >= d) return;
    const u32x4* wr = reinterpret_cast<const u32x4*>(w + (size_t)row * n);
    const int nch = n >> 3;                                   // 8-half chunks
    float mx = 0.f;
    bool finite = true;
    for (int c = (int)lane; c < nch; c += 64) {
        const u32x4 v = wr[c];
#pragma unroll
        for (int e = 0; e < 4; e++) {
            const h2 p = as_h2(v[e]);
            const float a = fabsf((float)p.x), b = fabsf((float)p.y);
            finite = finite && a <= 65504.f && b <= 65504.f;   // (false for inf and NaN)
            mx = fmaxf(mx, fmaxf(a, b));
        }
    }
    mx = wave_max(mx);
    finite = __all(finite);
    const float s = finite ? mx / 127.0f : 0.f;
    double se = 0.0, sw = 0.0, sq = 0.0;
    u32x2* qr = reinterpret_cast<u32x2*>(q8 + (size_t)row * n);
    for (int c = (int)lane; c < nch; c += 64) {
        const u32x4 v = wr[c];
        unsigned byte[8];
#pragma unroll
        for (int e = 0; e < 8; e++) {
            const h2 p = as_h2(v[e >> 1]);
            const float wf = finite ? (float)((e & 1) ? p.y : p.x) : 0.f;
            float q = s > 0.f ? rintf(wf / s) : 0.f;
            q = fminf(fmaxf(q, -127.f), 127.f);
            const double err = (double)wf - (double)s * (double)q;
            se += err * err;
            sw += (double)wf * (double)wf;
            sq += (double)q * (double)q;
            byte[e] = (unsigned)fabsf(q) | (q < 0.f ? 0x80u : 0u);
        }
        // word k: bytes 0, 2 = elements 4k, 4k + 1 (the even bytes), bytes 1, 3 = elements 4k + 2, 4k + 3
        u32x2 o;
        o[0] = byte[0] | (byte[2] << 8) | (byte[1] << 16) | (byte[3] << 24);
        o[1] = byte[4] | (byte[6] << 8) | (byte[5] << 16) | (byte[7] << 24);
        qr[c] = o;
    }
    se = wave_sum_f64(se); sw = wave_sum_f64(sw); sq = wave_sum_f64(sq);
    if (lane == 0) {
        const double E = sqrt(se), W = fmax(sqrt(sw), (double)s * sqrt(sq));
        scale[row] = s * 16777216.0f;
        ew[row] = finite ? (float)((E + CLS_SCREEN_GAMMA * W) * (1.0 + 1e-6)) : INFINITY;   // (a row with inf / NaN: always a candidate)
    }
}

// ---------------------------------------------------------------------------------------------------
// screen. NS = n / 512 as in cls_strip_kernel (the x staging is the same: one 8-half chunk per thread of waves 0 .. NS - 1); a row is NP = NS / 2 pieces
template <int NS, int D>
struct ScreenLds {
    static constexpr unsigned RING = 0;                                 // [16 waves][D] x 1 KiB
    static constexpr unsigned XN = RING + STRIP_WAVES * D * 1024u;      // [NS][64] x 16 B: the (normalised) input, chunk j = tid
    static constexpr unsigned PART = XN + NS * 1024u;                   // [NS * 64] rmsnorm chunk partials
    static constexpr unsigned PART2 = PART + NS * 256u;                 // [NS * 64] sums of squares of the staged chunks
    static constexpr unsigned LO = PART2 + NS * 256u;                   // [16] the waves' maxima of A - B
    static constexpr unsigned BYTES = LO + 64u;
};

template <int NS, bool NORM, int D>
__global__ void __launch_bounds__(STRIP_WAVES * 64) cls_screen_kernel(const u32x4* __restrict__ arg_x, const u32x4* __restrict__ arg_rms, const void* arg_q8, const unsigned qbytes,
                                                                     const unsigned rbase, const unsigned rrem, const float* __restrict__ scale, const float* __restrict__ ew,
                                                                     float2* __restrict__ ab, float* __restrict__ lo_out, u32x4* __restrict__ xn_out, unsigned* __restrict__ count,
                                                                     const int n, const unsigned row_bytes) {
    using L = ScreenLds<NS, D>;
    constexpr int NP = NS / 2;
    static_assert(D == 4 && D <= NP, "the first D pieces are the first row's");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const unsigned tid = threadIdx.x, lane = tid & 63u;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const unsigned r0 = blockIdx.x * rbase + (blockIdx.x < rrem ? blockIdx.x : rrem);
    const int nr = (int)(rbase + (blockIdx.x < rrem ? 1u : 0u));
    const int nu = (nr - wave + STRIP_WAVES - 1) / STRIP_WAVES;          // this wave's rows: r0 + wave + 16 i, i < nu <= 64 (cls_screen_shape)
    const int npieces = NP * nu;
    const unsigned voff = lane * 16u;
    const bool stager = wave < NS;

    u32x4 xraw = {0u, 0u, 0u, 0u}, wraw = {0u, 0u, 0u, 0u};
    float sc_l = 0.f, ew_l = 0.f;                                        // lane i: the constants of the wave's row i
    if (stager) {                                                        // asm loads: hipcc must not count them (it cannot see the DMA pieces behind them)
        const u32x4* px = arg_x + tid;
        asm volatile("global_load_dwordx4 %0, %1, off" : "=&v"(xraw) : "v"(px) : "memory");
        if (NORM) {
            const u32x4* pw = arg_rms + tid;
            asm volatile("global_load_dwordx4 %0, %1, off" : "=&v"(wraw) : "v"(pw) : "memory");
        }
    }
    if ((int)lane < nu) {
        const float* ps = scale + r0 + (unsigned)wave + 16u * lane;
        const float* pe = ew + r0 + (unsigned)wave + 16u * lane;
        asm volatile("global_load_dword %0, %1, off" : "=&v"(sc_l) : "v"(ps) : "memory");
        asm volatile("global_load_dword %0, %1, off" : "=&v"(ew_l) : "v"(pe) : "memory");
    }
    block_barrier_lds();      // the x loads are queued on this CU in front of every weight piece (the path returns in order)
    const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(arg_q8), 0, (int)qbytes, 0x00020000);
    const unsigned ring = L::RING + (unsigned)wave * (D * 1024u);
    const unsigned soff0 = (r0 + (unsigned)wave) * row_bytes;             // piece s of row i: soff0 + i * 16 rows + s * 1024
    auto issue2 = [&](int i, int s) { dma_piece(ring + (unsigned)((NP * i + s) & (D - 1)) * 1024u, voff, rw, soff0 + (unsigned)i * (16u * row_bytes) + (unsigned)s * 1024u); };
#pragma unroll
    for (int k = 0; k < D; k++)
        if (k < npieces) issue2(0, k);

    // ---- x chain: cls_strip_body's, and the norm of what it staged
    u32x4* xn = reinterpret_cast<u32x4*>(smem + L::XN);
    float* part = reinterpret_cast<float*>(smem + L::PART);
    float* part2 = reinterpret_cast<float*>(smem + L::PART2);
    float* wlo = reinterpret_cast<float*>(smem + L::LO);
    if (npieces >= D) asm volatile("s_waitcnt vmcnt(%4)" : "+v"(xraw), "+v"(wraw), "+v"(sc_l), "+v"(ew_l) : "n"(D) : "memory");   // all but the D weight pieces
    else asm volatile("s_waitcnt vmcnt(0)" : "+v"(xraw), "+v"(wraw), "+v"(sc_l), "+v"(ew_l) : : "memory");
    if (NORM) {
        if (stager) part[tid] = sumsq8(xraw, 0.f);
        block_barrier_lds();
    }
    if (stager) {
        u32x4 v = xraw;
        if (NORM) v = rms_apply8(v, wraw, rms_scale_from_partials<NS * 64>(part, NS * 64, n));
        xn[tid] = v;
        part2[tid] = sumsq8(v, 0.f);
    }
    block_barrier_lds();
    u32x4 X[NS];                                                         // piece s, this lane's 16 elements: chunks 2 (64 s + lane), + 1
#pragma unroll
    for (int s = 0; s < NP; s++) {
        X[2 * s] = xn[2 * (s * 64 + (int)lane)];
        X[2 * s + 1] = xn[2 * (s * 64 + (int)lane) + 1];
    }
    float xx = 0.f;
#pragma unroll
    for (int s = 0; s < NS; s++) xx += part2[s * 64 + lane];
    const float Xn = sqrtf(wave_sum(xx)) * (1.0f + 0.0009765625f);        // >= ||x||_2: a couple of dozen fp32 roundings against 2^-10
    const unsigned char* wbase = smem + ring + lane * 16u;

    float lomax = -INFINITY;
    for (int i = 0; i < nu; i++) {
        float sum = 0.f;
#pragma unroll
        for (int s = 0; s < NP; s++) {
            const int j = NP * i + s;
            if (j + D < npieces) wait_vmcnt<D - 1>(); else wait_vmcnt<0>();    // piece j has landed
            const u32x4 w = *reinterpret_cast<const u32x4*>(wbase + ((NP * i + s) & (D - 1)) * 1024);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                 // the read is done: the entry may be refilled
            if (j + D < npieces) issue2(i + (s + D) / NP, (s + D) % NP);
            float acc = 0.f;
#pragma unroll
            for (int k = 0; k < 4; k++) {       // sign-magnitude bytes as fp16 denormals m 2^-24 with the sign in bit 15: even bytes, then odd bytes
                const unsigned he = ((w[k] << 8) & 0x80008000u) | (w[k] & 0x007f007fu);
                const unsigned ho = (w[k] & 0x80008000u) | ((w[k] >> 8) & 0x007f007fu);
                const u32x4 xv = X[2 * s + (k >> 1)];
                acc = __builtin_amdgcn_fdot2(as_h2(he), as_h2(xv[2 * (k & 1)]), acc, false);
                acc = __builtin_amdgcn_fdot2(as_h2(ho), as_h2(xv[2 * (k & 1) + 1]), acc, false);
            }
            sum += acc;
        }
        const float t = wave_sum(sum);
        const float A = readlane_f(sc_l, i) * t;
        const float r = readlane_f(ew_l, i) * Xn;
        float B = ((r * (1.0f + 0.00048828125f) + 0.00048828125f * fabsf(A)) + 5.9604644775390625e-8f) * (1.0f + 9.5367431640625e-7f);
        if (!(fabsf(A) + B < 65504.f)) B = INFINITY;                           // fp16's overflow range, or a NaN: no claim, always a candidate
        const float lo = A - B;
        lomax = fmaxf(lomax, lo == lo ? lo : -INFINITY);
        if (lane == 0) ab[r0 + (unsigned)wave + 16u * (unsigned)i] = make_float2(A, B);
    }
    if (lane == 0) wlo[wave] = lomax;
    block_barrier_lds();
    if (tid == 0) {
        float m = wlo[0];
#pragma unroll
        for (int k = 1; k < STRIP_WAVES; k++) m = fmaxf(m, wlo[k]);
        lo_out[blockIdx.x] = m;
    }
    if (blockIdx.x == 0) {
        if (stager) xn_out[tid] = xn[tid];                                     // the refine launch multiplies with these bits
        if (tid == 0) {       // close the previous screened step's tally (its refine launch is complete: the launch boundary) and open this step's
            const unsigned cur = count[SCREEN_CUR];
            unsigned long long* wide = reinterpret_cast<unsigned long long*>(count);
            if (count[SCREEN_OPEN]) {
                count[SCREEN_LAST] = cur;
                if (cur > count[SCREEN_MAX]) count[SCREEN_MAX] = cur;
                wide[SCREEN_TOTAL / 2] += cur;
            }
            count[SCREEN_CUR] = 0u;
            count[SCREEN_OPEN] = 1u;
            wide[SCREEN_STEPS / 2] += 1ull;
        }
    }
}

// ---------------------------------------------------------------------------------------------------
// refine: the screen's grid and ownership of rows. The rare candidate row is read with plain loads (NS in flight per wave)
template <int NS>
__global__ void __launch_bounds__(STRIP_WAVES * 64) cls_refine_kernel(const u32x4* __restrict__ xn_in, const q4_half* __restrict__ w, const unsigned rbase, const unsigned rrem,
                                                                     const float2* __restrict__ ab, const float* __restrict__ lo_in, const int nblocks,
                                                                     q4_half* __restrict__ out, unsigned* __restrict__ count, const int n) {
    __shared__ __attribute__((aligned(16))) u32x4 xn[NS * 64];
    const unsigned tid = threadIdx.x, lane = tid & 63u;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const unsigned r0 = blockIdx.x * rbase + (blockIdx.x < rrem ? blockIdx.x : rrem);
    const int nr = (int)(rbase + (blockIdx.x < rrem ? 1u : 0u));
    const int nu = (nr - wave + STRIP_WAVES - 1) / STRIP_WAVES;          // <= 64
    if (tid < (unsigned)(NS * 64)) xn[tid] = xn_in[tid];
    float g = -INFINITY;
    for (int b = (int)lane; b < nblocks; b += 64) g = fmaxf(g, lo_in[b]);
    const float G = wave_max(g);
    bool cand = false;
    if ((int)lane < nu) {
        const unsigned row = r0 + (unsigned)wave + 16u * lane;
        const float2 v = ab[row];
        cand = !(v.x + v.y < G);                                         // (a NaN makes a candidate)
        if (!cand) out[row] = (q4_half)0xfc00u;                          // -inf
    }
    unsigned long long mask = __ballot(cand);
    __syncthreads();
    u32x4 X[NS];
#pragma unroll
    for (int s = 0; s < NS; s++) X[s] = xn[s * 64 + lane];
    if (lane == 0 && mask) atomicAdd(count + SCREEN_CUR, (unsigned)__popcll(mask));
    while (mask) {
        const int i = __builtin_ctzll(mask);
        mask &= mask - 1ull;
        const unsigned row = r0 + (unsigned)wave + 16u * (unsigned)i;
        const u32x4* wr = reinterpret_cast<const u32x4*>(w + (size_t)row * n);
        u32x4 W[NS];
#pragma unroll
        for (int s = 0; s < NS; s++) W[s] = ld_nt(wr + s * 64 + lane);
        float sum = 0.f;
#pragma unroll
        for (int s = 0; s < NS; s++) {                                   // cls_strip_body's arithmetic, in its order
            float acc = 0.f;
#pragma unroll
            for (int e = 0; e < 4; e++) acc = __builtin_amdgcn_fdot2(as_h2(W[s][e]), as_h2(X[s][e]), acc, false);
            sum += acc;
        }
        float t = wave_sum(sum);
        t *= 1.0f;
        if (lane == 0) out[row] = f2h(t);
    }
}

// ---------------------------------------------------------------------------------------------------
bool cls_screen_shape(int n, int d) {
    return classifier_runs_as_strips(n, d) && divUp(d, cu_count()) <= 64 * STRIP_WAVES;
}
int cls_screen_prepare() {
    static int prepared_device = -1;
    int dev = -1;
    if (hipGetDevice(&dev) == hipSuccess && dev == prepared_device) return Q4_OK;
    int rc = Q4_OK;
    if (!rc) rc = lds_opt_in((const void*)cls_screen_kernel<8, true, CLS_D>, ScreenLds<8, CLS_D>::BYTES);
    if (!rc) rc = lds_opt_in((const void*)cls_screen_kernel<8, false, CLS_D>, ScreenLds<8, CLS_D>::BYTES);
    if (!rc) rc = lds_opt_in((const void*)cls_screen_kernel<10, true, CLS_D>, ScreenLds<10, CLS_D>::BYTES);
    if (!rc) rc = lds_opt_in((const void*)cls_screen_kernel<10, false, CLS_D>, ScreenLds<10, CLS_D>::BYTES);
    if (!rc) prepared_device = dev;
    return rc;
}

static size_t up256(size_t v) { return (v + 255) / 256 * 256; }
int cls_screen_build(ClsScreen* sc, const q4_half* wcls, int n, int d) {
    *sc = ClsScreen{};
    if (!cls_screen_shape(n, d)) return Q4_ERR_UNSUPPORTED_SIZE;
    Q4_TRY(cls_screen_prepare());
    const int nb = cu_count();
    const size_t b_q8 = up256((size_t)d * n), b_row = up256((size_t)d * sizeof(float)), b_ab = up256((size_t)d * sizeof(float2)), b_lo = up256((size_t)nb * sizeof(float)),
                 b_xn = up256((size_t)n * sizeof(q4_half)), b_cnt = 256;
    void* base = nullptr;
    if (hipMalloc(&base, b_q8 + 2 * b_row + b_ab + b_lo + b_xn + b_cnt) != hipSuccess) { (void)hipGetLastError(); return Q4_ERR_ALLOC; }
    char* c = (char*)base;
    sc->base = base;
    sc->q8 = (unsigned char*)c; c += b_q8;
    sc->scale = (float*)c; c += b_row;
    sc->ew = (float*)c; c += b_row;
    sc->ab = (float2*)c; c += b_ab;
    sc->lo = (float*)c; c += b_lo;
    sc->xn = (q4_half*)c; c += b_xn;
    sc->count = (unsigned*)c;
    sc->n = n; sc->d = d; sc->blocks = nb;
    hipError_t e = hipMemsetAsync(sc->ab, 0, b_ab + b_lo + b_xn + b_cnt, g_stream);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(cls_screen_build_kernel, dim3((unsigned)divUp(d, 4)), dim3(256), 0, g_stream, wcls, sc->q8, sc->scale, sc->ew, n, d);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(g_stream);
    if (e != hipSuccess) { cls_screen_free(sc); return hip_fail(e, "cls_screen_build", __FILE__, __LINE__); }
    return Q4_OK;
}
void cls_screen_free(ClsScreen* sc) {
    if (sc->base) (void)hipFree(sc->base);
    *sc = ClsScreen{};
}

template <int NS>
static int launch_cls_screen_n(const ClsScreen& sc, q4_half* logits, const q4_half* x, const q4_half* rms_w, const q4_half* wcls) {
    const unsigned nb = (unsigned)sc.blocks;
    constexpr size_t smem = ScreenLds<NS, CLS_D>::BYTES;
    const unsigned rbase = (unsigned)sc.d / nb, rrem = (unsigned)sc.d % nb;
    if (rms_w)
        Q4_LAUNCH((cls_screen_kernel<NS, true, CLS_D>), dim3(nb), dim3(STRIP_WAVES * 64), smem, reinterpret_cast<const u32x4*>(x), reinterpret_cast<const u32x4*>(rms_w),
                  (const void*)sc.q8, (unsigned)((size_t)sc.d * sc.n), rbase, rrem, (const float*)sc.scale, (const float*)sc.ew, sc.ab, sc.lo, reinterpret_cast<u32x4*>(sc.xn), sc.count,
                  sc.n, (unsigned)sc.n);
    else
        Q4_LAUNCH((cls_screen_kernel<NS, false, CLS_D>), dim3(nb), dim3(STRIP_WAVES * 64), smem, reinterpret_cast<const u32x4*>(x), reinterpret_cast<const u32x4*>(rms_w),
                  (const void*)sc.q8, (unsigned)((size_t)sc.d * sc.n), rbase, rrem, (const float*)sc.scale, (const float*)sc.ew, sc.ab, sc.lo, reinterpret_cast<u32x4*>(sc.xn), sc.count,
                  sc.n, (unsigned)sc.n);
    Q4_LAUNCH_CHECK();
    Q4_LAUNCH((cls_refine_kernel<NS>), dim3(nb), dim3(STRIP_WAVES * 64), 0, reinterpret_cast<const u32x4*>(sc.xn), wcls, rbase, rrem, (const float2*)sc.ab, (const float*)sc.lo,
              (int)nb, logits, sc.count, sc.n);
    Q4_LAUNCH_CHECK();
    return Q4_OK;
}
int launch_cls_screen(const ClsScreen& sc, q4_half* logits, const q4_half* x, const q4_half* rms_w, const q4_half* wcls) {
    if (!sc.base || sc.blocks != cu_count() || !cls_screen_shape(sc.n, sc.d)) return Q4_ERR_UNSUPPORTED_SIZE;   // (the caller asked cls_screen_shape first: no quiet other path)
    Q4_TRY(cls_screen_prepare());
    return sc.n == 4096 ? launch_cls_screen_n<8>(sc, logits, x, rms_w, wcls) : launch_cls_screen_n<10>(sc, logits, x, rms_w, wcls);
}

}  // namespace q4

using namespace q4;

extern "C" {

// Op-level entry point (tests, tools): the screen, the refinement and the argmax of ONE input against an fp16 matrix [d][n] on the device, with a
// screening copy built and freed inside the call. x, w, rms_w (may be null: x is taken as it is) are device pointers; the outputs are HOST arrays
// (any may be null): the token, A and B [d] floats, the refined logits [d] halves, the number of candidate rows.
int q4_greedy_screen_op(const q4_half* x, const q4_half* w, int n, int d, const q4_half* rms_w, int* token, float* A, float* B, q4_half* refined, int* candidates) {
    if (!x || !w || n <= 0 || d <= 0) return Q4_ERR_ARG;
    if (!cls_screen_shape(n, d)) return Q4_ERR_UNSUPPORTED_SIZE;
    ClsScreen sc;
    { const int rc = cls_screen_build(&sc, w, n, d); if (rc) return rc; }
    struct Tmp { q4_half* logits; int* word; } tmp = {nullptr, nullptr};   // the logits, and {token ring [2], position, position}
    int rc = Q4_OK;
    if (hipMalloc((void**)&tmp.logits, (size_t)d * sizeof(q4_half)) != hipSuccess || hipMalloc((void**)&tmp.word, 4 * sizeof(int)) != hipSuccess) { (void)hipGetLastError(); rc = Q4_ERR_ALLOC; }
    if (!rc && hipMemsetAsync(tmp.word, 0, 4 * sizeof(int), g_stream) != hipSuccess) rc = Q4_ERR_HIP;
    if (!rc) rc = launch_cls_screen(sc, tmp.logits, x, rms_w, w);
    if (!rc) rc = q4_argmax(tmp.logits, d, tmp.word, tmp.word + 2, tmp.word + 3, 1);      // writes ring[1], positions -> 1
    if (!rc && hipStreamSynchronize(g_stream) != hipSuccess) rc = Q4_ERR_HIP;
    if (!rc) {
        std::vector<float2> ab((size_t)d);
        int word[4] = {0, 0, 0, 0};
        unsigned cnt[SCREEN_WORDS] = {};
        if (hipMemcpy(ab.data(), sc.ab, (size_t)d * sizeof(float2), hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(word, tmp.word, sizeof(word), hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(cnt, sc.count, sizeof(cnt), hipMemcpyDeviceToHost) != hipSuccess ||
            (refined && hipMemcpy(refined, tmp.logits, (size_t)d * sizeof(q4_half), hipMemcpyDeviceToHost) != hipSuccess))
            rc = Q4_ERR_HIP;
        for (int r = 0; r < d && !rc; r++) {
            if (A) A[r] = ab[r].x;
            if (B) B[r] = ab[r].y;
        }
        if (token) *token = word[1];
        if (candidates) *candidates = (int)cnt[SCREEN_CUR];
    }
    if (rc == Q4_ERR_HIP) (void)hipGetLastError();
    if (tmp.logits) (void)hipFree(tmp.logits);
    if (tmp.word) (void)hipFree(tmp.word);
    cls_screen_free(&sc);
    return rc;
}

}  // extern "C"
