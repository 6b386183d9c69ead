// attention_kv8.h -- MultiHeadAttention over an FP8 (OCP e4m3fn) K / V cache: the opt-in cache format Q4_KV_FP8.
// A cache row of one (position, kv head) is head_size e4m3 bytes plus ONE signed exponent byte e: the smallest integer in [-15, 7] with
// amax <= 448 * 2^e; element x is stored as e4m3_rne(clamp(float(x) * 2^-e, +-448)). Every dequantised value byte * 2^e is exactly an
// fp16 number, so the mode computes "the fp16 attention over a cache whose rows were replaced by their round trip": the rounding points
// are attention.h's (scores through fp16, one-pass probabilities through fp16, fp32 probabilities in the split-context form). The row's
// exponent folds into the score ((sum q . k8) * 2^e) and into the probability in front of P . V -- exact scalings, no per-element multiply.
// A row is head_size bytes = LPR lanes x 16 B, so one wave instruction fetches 64 / LPR positions: 8 of a 128-wide head.
//
// THE LAUNCH APPENDS. The QKV launch in front of it leaves this position's K (rotated) and V as fp16 in two staging rows; every block
// that needs position `pos` quantises the staging row in registers (the same bits in every block) and uses the round-tripped values;
// exactly one block per kv head stores the bytes and the exponent. No block reads position `pos` from the cache (every cache load is a
// buffer load bounded at `pos` rows, every exponent load is guarded by t < pos): no race inside the launch and no extra launch.
#pragma once
#include "attention.h"

namespace q4 {

constexpr int KV8_E_MIN = -15, KV8_E_MAX = 7;

struct Kv8Args {
    q4_half* output;             // [n_heads * head_size]
    const q4_half* q;
    uint8_t* k8;                 // [seq_len][kv_dim] e4m3 bytes, already offset to the layer
    uint8_t* v8;
    int8_t* k_exp;               // [n_kv_heads][exp_stride] row exponents, already offset to the layer
    int8_t* v_exp;
    const q4_half* k_row;        // [kv_dim] this position's K (rotated) and V as the QKV launch left them
    const q4_half* v_row;
    int head_size, kv_mul, kv_dim, exp_stride;
    const int* pPos;
    float alpha;
    int lds_scores;              // one-pass form: fp32 score slots in LDS (the sequence-length bin)
    float* partials;             // split-context form: [heads][nsp][head_size + ATT_REC_PAD] flash-decode records (attention.h)
    unsigned* arrive;            // ... [heads] arrival counters, or null: attention_combine_kernel merges in a second launch
};

__device__ __forceinline__ float kv8_pow2(int e) { return as_f((127 + e) << 23); }   // e in [-15, 15]: a normal fp32

// this lane's 16 elements of a staging row (row16 = the row + head offset + sub * 16) -> 16 e4m3 bytes and the row's exponent. The LPR
// lanes that share a head's row hold its slices; every group of LPR lanes of the wave holds the same row, so xor shuffles below LPR
// stay inside a row and the loop below is wave-uniform.
template <int LPR>
__device__ __forceinline__ void kv8_quantise(const q4_half* row16, u32x4& bytes, int& e) {
    const u32x4 lo = *reinterpret_cast<const u32x4*>(row16), hi = *reinterpret_cast<const u32x4*>(row16 + 8);
    float x[16];
#pragma unroll
    for (int d = 0; d < 4; d++) {
        const h2 a = as_h2(lo[d]), b = as_h2(hi[d]);
        x[2 * d] = (float)a.x; x[2 * d + 1] = (float)a.y;
        x[8 + 2 * d] = (float)b.x; x[8 + 2 * d + 1] = (float)b.y;
    }
    float amax = 0.f;
#pragma unroll
    for (int i = 0; i < 16; i++) amax = fmaxf(amax, fabsf(x[i]));
#pragma unroll
    for (int o = 1; o < LPR; o <<= 1) amax = fmaxf(amax, __shfl_xor(amax, o));
    e = KV8_E_MIN;
    float lim = 448.f * 0x1p-15f;                       // exact comparisons against 448 * 2^e, no logarithm
    while (e < KV8_E_MAX && amax > lim) { e++; lim *= 2.f; }
    const float inv = kv8_pow2(-e);                     // the scaling is exact in fp32
#pragma unroll
    for (int d = 0; d < 4; d++) {
        float c[4];
#pragma unroll
        for (int k = 0; k < 4; k++) c[k] = fminf(fmaxf(x[4 * d + k] * inv, -448.f), 448.f);   // rows with amax > 57344 saturate
        int w = 0;
        w = __builtin_amdgcn_cvt_pk_fp8_f32(c[0], c[1], w, false);                          // v_cvt_pk_fp8_f32: RNE, subnormals kept
        w = __builtin_amdgcn_cvt_pk_fp8_f32(c[2], c[3], w, true);
        bytes[d] = (unsigned)w;
    }
}

// sum over this lane's 16 elements of q . k8: the bytes widen to fp16 exactly (v_cvt_scalef32_pk_f16_fp8, scale 1), the products and the sum are
// attention.h's v_dot2c_f32_f16 chain -- 16 VALU per 16 bytes, against 24 for v_cvt_pk_f32_fp8 + fma
__device__ __forceinline__ float kv8_dot16(const u32x4 kb, const u32x4 q0, const u32x4 q1) {
    float s = 0.f;
#pragma unroll
    for (int d = 0; d < 4; d++) {
        const h2 lo = __builtin_bit_cast(h2, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(kb[d], 1.0f, false));
        const h2 hi = __builtin_bit_cast(h2, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(kb[d], 1.0f, true));
        const unsigned qa = d < 2 ? q0[2 * d] : q1[2 * d - 4], qb = d < 2 ? q0[2 * d + 1] : q1[2 * d - 3];
        s = __builtin_amdgcn_fdot2(lo, as_h2(qa), s, false);
        s = __builtin_amdgcn_fdot2(hi, as_h2(qb), s, false);
    }
    return s;
}

// acc[0..16) += p * v8 (p already carries the row's 2^e)
__device__ __forceinline__ void kv8_axpy16(float (&acc)[16], const u32x4 vb, const float p) {
#pragma unroll
    for (int d = 0; d < 4; d++) {
        const auto lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)vb[d], false);
        const auto hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)vb[d], true);
        acc[4 * d] = __builtin_fmaf(lo[0], p, acc[4 * d]);
        acc[4 * d + 1] = __builtin_fmaf(lo[1], p, acc[4 * d + 1]);
        acc[4 * d + 2] = __builtin_fmaf(hi[0], p, acc[4 * d + 2]);
        acc[4 * d + 3] = __builtin_fmaf(hi[1], p, acc[4 * d + 3]);
    }
}

// the 64 / LPR rows of a wave summed into its first LPR lanes, which leave the wave's partial of the head in LDS
template <int LPR>
__device__ __forceinline__ void kv8_store_partial(float (&acc)[16], float* outp_wave, const unsigned lane, const int sub) {
#pragma unroll
    for (int e = 0; e < 16; e++) {
        float v = acc[e];
        v += __shfl_xor(v, 32);
        v += __shfl_xor(v, 16);
        if (LPR <= 8) v += __shfl_xor(v, 8);
        if (LPR <= 4) v += __shfl_xor(v, 4);
        acc[e] = v;
    }
    if (lane < (unsigned)LPR) {
#pragma unroll
        for (int e = 0; e < 16; e++) outp_wave[sub * 16 + e] = acc[e];
    }
}

// the one block of a kv head that appends: its first LPR lanes store the row's bytes, lane 0 the two exponents
template <int LPR>
__device__ __forceinline__ void kv8_append(const Kv8Args& a, const int kvh, const int pos, const unsigned tid, const size_t hoff,
                                           const u32x4 kq, const int ke, const u32x4 vq, const int ve) {
    if (tid < (unsigned)LPR) {
        *reinterpret_cast<u32x4*>(a.k8 + (size_t)pos * a.kv_dim + hoff) = kq;
        *reinterpret_cast<u32x4*>(a.v8 + (size_t)pos * a.kv_dim + hoff) = vq;
        if (tid == 0) {
            a.k_exp[(size_t)kvh * a.exp_stride + pos] = (int8_t)ke;
            a.v_exp[(size_t)kvh * a.exp_stride + pos] = (int8_t)ve;
        }
    }
}

// ---- the short bins: ONE block per head, attention_kernel's three passes (scores -> LDS, softmax statistics, P . V) ------------------------------
// One kernel, two instantiations -- one statement of the arithmetic:
//  * ROW false, the step's launch: block h is head h at position *a.pPos; this position's row is quantised from the staging rows, used from registers
//    (`cur`) and appended behind the head's output.
//  * ROW true, the row form of a prompt or verify pass (prompt_pass_kv8.hip): block b is (token b / n_heads, head b % n_heads) of rows `dim` halves
//    apart in a.q / a.output with positions a.pPos[token]; the launch in front has appended the tokens' rows, so every row up to and including the
//    position comes from the cache -- the bytes and exponents the step holds in registers -- and nothing is stored but the output. a.k_row / a.v_row
//    are not read.
// Either way the resource ends where the block's own rows end: what lies above reads as zeros. (The flag is a kernel template argument and not a
// __device__ body called by two kernels: moving the body behind a function boundary changed the step kernel's register allocation and address
// arithmetic; this way the step's instruction stream is what it was before the flag existed.)
template <int LPR, int U = 4, int NW = ATT_NW, bool ROW = false>
__global__ void __launch_bounds__(NW * 64) attention_kv8_kernel(const Kv8Args a0) {
    static_assert(LPR == 4 || LPR == 8 || LPR == 16, "head sizes 64, 128, 256");
    constexpr int R = 64 / LPR;                              // positions per wave instruction
    constexpr int stride = NW * R, group = stride * U;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float* red_max = reinterpret_cast<float*>(smem);         // [16]
    float* red_sum = red_max + 16;                           // [16]
    float* outp = red_sum + 16;                              // [NW][head_size] output partials
    float* sc = outp + NW * a0.head_size;                    // [lds_scores] scores, then exps
    Kv8Args a = a0;
    int h = blockIdx.x;
    if constexpr (ROW) {
        const int n_heads = a0.kv_dim / a0.head_size * a0.kv_mul, tok = blockIdx.x / n_heads;
        h = blockIdx.x - tok * n_heads;
        a.pPos = a0.pPos + tok;
        a.q = a0.q + (size_t)tok * n_heads * a0.head_size;
        a.output = a0.output + (size_t)tok * n_heads * a0.head_size;
    }
    const int head_size = a.head_size, kv_dim = a.kv_dim, kvh = h / a.kv_mul;
    const unsigned tid = threadIdx.x, lane = tid & 63u;
    const int wave = tid >> 6, row = lane / LPR, sub = lane % LPR;
    const size_t hoff = (size_t)kvh * head_size + sub * 16;  // this lane's 16-byte slice inside a cache row
    if (NW < 16 && tid >= NW && tid < 16) { red_max[tid] = -INFINITY; red_sum[tid] = 0.f; }
    const int pos = __builtin_amdgcn_readfirstlane(*a.pPos);
    const int size = pos + 1;
    const int cached = ROW ? size : pos;                     // rows the cache holds for this block
    const u32x4 q0 = *reinterpret_cast<const u32x4*>(a.q + (size_t)h * head_size + sub * 16);
    const u32x4 q1 = *reinterpret_cast<const u32x4*>(a.q + (size_t)h * head_size + sub * 16 + 8);
    u32x4 kq, vq;
    int ke, ve;
    if constexpr (ROW) {
        kq = vq = (u32x4){0u, 0u, 0u, 0u};
        ke = ve = 0;
    } else {
        kv8_quantise<LPR>(a.k_row + hoff, kq, ke);
        kv8_quantise<LPR>(a.v_row + hoff, vq, ve);
    }
    // bounded at `cached` rows: a row at or past the bound comes back as zeros without a memory request
    const __amdgpu_buffer_rsrc_t rk = __builtin_amdgcn_make_buffer_rsrc((void*)a.k8, 0, (unsigned)cached * (unsigned)kv_dim, 0x00020000);
    const __amdgpu_buffer_rsrc_t rv = __builtin_amdgcn_make_buffer_rsrc((void*)a.v8, 0, (unsigned)cached * (unsigned)kv_dim, 0x00020000);
    const int8_t* kex = a.k_exp + (size_t)kvh * a.exp_stride;
    const int8_t* vex = a.v_exp + (size_t)kvh * a.exp_stride;

    // ---- pass 1: scores (loop bounds are wave-uniform so the DPP row sums always see full rows)
    float wmax = -INFINITY;
    for (int g0 = 0; g0 < size; g0 += group) {
        u32x4 kb[U];
        int ex[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            const int t = g0 + wave * R + row + u * stride;
            kb[u] = __builtin_amdgcn_raw_buffer_load_b128(rk, (unsigned)t * (unsigned)kv_dim + (unsigned)hoff, 0, 0);
            ex[u] = t < cached ? (int)kex[t] : 0;
        }
#pragma unroll
        for (int u = 0; u < U; u++) {
            const int t = g0 + wave * R + row + u * stride;
            const bool cur = !ROW && t == pos;
            float s = row_sum<LPR>(kv8_dot16(cur ? kq : kb[u], q0, q1));
            s = round_h(s * kv8_pow2(cur ? ke : ex[u]) * a.alpha);     // the exponent: an exact scaling; then attention.h's rounding point
            if (t < size) {
                wmax = fmaxf(wmax, s);
                if (sub == 0) sc[t] = s;
            }
        }
    }
    wmax = wave_max(wmax);
    if (lane == 0) red_max[wave] = wmax;
    __syncthreads();

    // ---- softmax statistics: attention_body's, the no-smem rounding of the bins past 8192 included
    const bool no_smem = a.lds_scores > 8192;
    const float m = row16_max(red_max[lane & 15]);
    float sum = 0.f;
    for (int t = tid; t < size; t += NW * 64) {
        const float e = expf(sc[t] - m);
        sc[t] = no_smem ? round_h(e) : e;
        sum += e;
    }
    sum = wave_sum(sum);
    if (lane == 0) red_sum[wave] = sum;
    __syncthreads();
    sum = row16_sum(red_sum[lane & 15]);
    const float inv_sum = 1.0f / sum;

    // ---- pass 2: att . V
    float acc[16];
#pragma unroll
    for (int e = 0; e < 16; e++) acc[e] = 0.f;
    for (int g0 = 0; g0 < size; g0 += group) {
        u32x4 vb[U];
        int ex[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            const int t = g0 + wave * R + row + u * stride;
            vb[u] = __builtin_amdgcn_raw_buffer_load_b128(rv, (unsigned)t * (unsigned)kv_dim + (unsigned)hoff, 0, 0);
            ex[u] = t < cached ? (int)vex[t] : 0;
        }
#pragma unroll
        for (int u = 0; u < U; u++) {
            const int t = g0 + wave * R + row + u * stride;
            const bool cur = !ROW && t == pos;
            const float p = t < size ? round_h(sc[t] * inv_sum) * kv8_pow2(cur ? ve : ex[u]) : 0.f;
            kv8_axpy16(acc, cur ? vq : vb[u], p);
        }
    }
    kv8_store_partial<LPR>(acc, outp + wave * head_size, lane, sub);
    __syncthreads();
    for (int n = tid; n < head_size; n += NW * 64) {
        float part[NW];
#pragma unroll
        for (int w = 0; w < NW; w++) part[w] = outp[w * head_size + n];
        float s = 0.f;
#pragma unroll
        for (int w = 0; w < NW; w++) s += part[w];
        a.output[(size_t)h * head_size + n] = f2h(s);
    }
    if constexpr (!ROW) {
        if (h % a.kv_mul == 0) kv8_append<LPR>(a, kvh, pos, tid, hoff, kq, ke, vq, ve);
    }
}

// ---- long contexts: one block per (head, chunk of NW * (64 / LPR) * U positions), attention_split_kernel's flash-decode records in the same layout, so
// that the last-arriver merge on the head's counter and attention_combine_kernel serve as they are
template <int LPR, int U, int NW = ATT_NW>
__global__ void __launch_bounds__(NW * 64) attention_kv8_split_kernel(const Kv8Args a) {
    static_assert(LPR == 4 || LPR == 8 || LPR == 16, "head sizes 64, 128, 256");
    constexpr int R = 64 / LPR;
    constexpr int stride = NW * R, CHUNK = stride * U;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float* red_max = reinterpret_cast<float*>(smem);
    float* red_sum = red_max + 16;
    float* outp = red_sum + 16;                              // [NW][head_size]
    __shared__ int is_last;
    const int h = blockIdx.x, sp = blockIdx.y, nsp = gridDim.y;
    const int head_size = a.head_size, kv_dim = a.kv_dim, kvh = h / a.kv_mul;
    const int rec = head_size + ATT_REC_PAD;
    const unsigned tid = threadIdx.x, lane = tid & 63u;
    const int wave = tid >> 6, row = lane / LPR, sub = lane % LPR;
    const size_t hoff = (size_t)kvh * head_size + sub * 16;
    const int pos = __builtin_amdgcn_readfirstlane(*a.pPos);
    const int size = pos + 1;
    const int t_base = sp * CHUNK;
    const SplitArgs sa = {a.partials, a.q, nullptr, nullptr, head_size, a.kv_mul, kv_dim, a.pPos, a.alpha, a.output, a.arrive, nullptr};
    if (NW < 16 && tid >= NW && tid < 16) { red_max[tid] = -INFINITY; red_sum[tid] = 0.f; }
    if (t_base < size) {
        const u32x4 q0 = *reinterpret_cast<const u32x4*>(a.q + (size_t)h * head_size + sub * 16);
        const u32x4 q1 = *reinterpret_cast<const u32x4*>(a.q + (size_t)h * head_size + sub * 16 + 8);
        const __amdgpu_buffer_rsrc_t rk = __builtin_amdgcn_make_buffer_rsrc((void*)a.k8, 0, (unsigned)pos * (unsigned)kv_dim, 0x00020000);
        const __amdgpu_buffer_rsrc_t rv = __builtin_amdgcn_make_buffer_rsrc((void*)a.v8, 0, (unsigned)pos * (unsigned)kv_dim, 0x00020000);
        const int8_t* kex = a.k_exp + (size_t)kvh * a.exp_stride;
        const int8_t* vex = a.v_exp + (size_t)kvh * a.exp_stride;
        // request order: q, every K row, every V row, the exponents (one memory latency for the chunk)
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
            const int t = t_base + wave * R + row + u * stride;
            ek[u] = t < pos ? (int)kex[t] : 0;
            ev[u] = t < pos ? (int)vex[t] : 0;
        }
        const bool holds_pos = pos < t_base + CHUNK;         // (block-uniform) the chunk of the position: its row comes from the staging rows
        u32x4 kq = {0u, 0u, 0u, 0u}, vq = {0u, 0u, 0u, 0u};
        int ke = 0, ve = 0;
        if (holds_pos) {
            kv8_quantise<LPR>(a.k_row + hoff, kq, ke);
            kv8_quantise<LPR>(a.v_row + hoff, vq, ve);
#pragma unroll
            for (int u = 0; u < U; u++)
                if (t_base + wave * R + row + u * stride == pos) { kb[u] = kq; vb[u] = vq; ek[u] = ke; ev[u] = ve; }
        }
        float scv[U];
        float wmax = -INFINITY;
#pragma unroll
        for (int u = 0; u < U; u++) {
            const int t = t_base + wave * R + row + u * stride;
            float s = row_sum<LPR>(kv8_dot16(kb[u], q0, q1));
            s = round_h(s * kv8_pow2(ek[u]) * a.alpha);
            scv[u] = t < size ? s : -INFINITY;
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
            const float p = expf(scv[u] - m);                // fp32 probabilities here, 0 for masked positions
            if (sub == 0) lsum += p;
            kv8_axpy16(acc, vb[u], p * kv8_pow2(ev[u]));
        }
        lsum = wave_sum(lsum);
        if (lane == 0) red_sum[wave] = lsum;
        kv8_store_partial<LPR>(acc, outp + wave * head_size, lane, sub);
        __syncthreads();
        const float l = row16_sum(red_sum[lane & 15]);
        split_store_record<false, NW>(sa, Handoff{}, outp, m, l, h, sp, nsp);
        if (holds_pos && h % a.kv_mul == 0) kv8_append<LPR>(a, kvh, pos, tid, hoff, kq, ke, vq, ve);
    } else if (tid == 0) {                                   // a chunk entirely in the future: the neutral record (m = -inf, l = 0)
        const f32x4 r4 = {-INFINITY, 0.f, 0.f, 0.f};
        float* dst = a.partials + ((size_t)h * nsp + sp) * rec + head_size;
        if (a.arrive) asm volatile("global_store_dwordx4 %0, %1, off sc1" ::"v"(dst), "v"(r4) : "memory");
        else *reinterpret_cast<f32x4*>(dst) = r4;
    }
    if (a.arrive == nullptr) return;
    // ---- last-arriver merge (attention_split_body's): record drained to memory, then ONE returning arrival per block
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0) {
        const unsigned old = __hip_atomic_fetch_add(a.arrive + h, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        is_last = old == (unsigned)nsp - 1u;
        if (is_last) __hip_atomic_store(a.arrive + h, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
    if (!is_last) return;
    for (int n = tid; n < head_size; n += NW * 64)
        combine_partials<true>(a.output + (size_t)h * head_size, a.partials + (size_t)h * nsp * rec, head_size, nsp, n);
}

}  // namespace q4
