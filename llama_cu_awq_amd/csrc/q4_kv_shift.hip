// q4_kv_shift.hip -- context shift: one launch that moves the K / V rows of positions [n_keep + D, n_pos) down by D = n_discard positions IN PLACE, in
// every layer, and rotates every moved K row by -D positions (cached K rows are stored rotated: pairs (i, i + head_size/2)). Not in the reference.
// The move overlaps itself whenever more rows move than are discarded, so q4_kv_copy.hip refuses it; a scratch copy of the rows would be gigabytes.
// Ownership goes BY COLUMN: destination (r - D, col) depends on source (r, col) and on nothing else, so a work item owns a fixed (K | V, layer, 16-byte
// column chunk) and walks the positions n_keep + D .. n_pos - 1 in ASCENDING order, storing to r - D. Every row it overwrites lies below the row it is
// processing: it was either discarded or loaded AND consumed by this very item earlier in program order (its data had arrived, or it could not have been
// stored). Loads run ahead only upward, KS_U rows deep. No atomics, no flags, no ordering beyond the stream's; one launch for any D, D = 1 included.
// Items that share a cache line write disjoint bytes of it.
//   fp16: an item holds the two chunks of eight pairs, [8j, 8j + 8) and [head_size/2 + 8j, ...) of one head, so a K rotation needs no other lane; V items
//         hold the same two chunks and store them as they are. head_size % 16 != 0 (or a base that is not 16-byte aligned): a scalar kernel, one pair
//         of halves per item.
//   FP8:  the LPR = head_size/16 lanes of a head's row walk together (attention_kv8.h); the pair partner's bytes are one xor shuffle away, at LPR/2;
//         a K row is dequantised (byte * 2^e: exactly fp16), rotated, rounded to half and quantised again by the format's own rule (amax by an xor
//         reduction inside the LPR lanes); lane 0 of the row stores the exponent. V bytes and V exponents move as they are, in the same launch.
// The arithmetic of a pair (a, b) = (k[i], k[i + head_size/2]) with (c, s) = row D of the rotation table at i, every operation ONE IEEE fp32 operation:
//   k'[i] = half_rne((a * c) + (b * s))      k'[i + head_size/2] = half_rne((b * c) - (a * s))        (tests/context_shift_ref.py restates it in numpy)
// Loads and stores are non-temporal (the rows are used once and must not push the weights out of the Infinity Cache); every offset is 64-bit.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "q4_device.h"
#include "q4_model.h"
using namespace q4;

namespace {

constexpr int KS_T = 64;                 // one wave per block: a 7B model has 256 waves of items, one per CU
constexpr int KS_U = 16;                 // rows in flight per item: 16 x 2 KiB per wave (fp16), what keeps a CU streaming (tests/test_kv_shift_gpu.py states it too)
constexpr int KS_BLOCKS_PER_CU = 8;
constexpr int KS_E_MIN = -15, KS_E_MAX = 7;          // the FP8 format's exponent range (attention_kv8.h)

__device__ __forceinline__ float pow2f(int e) { return as_f((127 + e) << 23); }   // e in [-15, 15]: a normal fp32

struct ShiftArgs {
    char* k; char* v;
    int8_t* k_exp; int8_t* v_exp;
    const float2* cs;                    // [head_size/2] (cos, sin) of D positions
    int n_layers, seq_len, n_kv_heads, head_size;
    int r0, n_pos, D;                    // the first row that moves (n_keep + D), one past the last, the distance
};

__device__ __forceinline__ u32x4 ld16(const char* p) { return __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p)); }
__device__ __forceinline__ void st16(char* p, u32x4 v) { __builtin_nontemporal_store(v, reinterpret_cast<u32x4*>(p)); }

// one pair, rotated by -D: every operation rounds once (no contraction)
__device__ __forceinline__ float rot_lo(float a, float b, float c, float s) { return __fadd_rn(__fmul_rn(a, c), __fmul_rn(b, s)); }
__device__ __forceinline__ float rot_hi(float a, float b, float c, float s) { return __fsub_rn(__fmul_rn(b, c), __fmul_rn(a, s)); }

// eight pairs held as two 16-byte chunks of halves
__device__ __forceinline__ void rotate8(u32x4& lo, u32x4& hi, const float (&c)[8], const float (&s)[8]) {
#pragma unroll
    for (int d = 0; d < 4; d++) {
        const h2 A = as_h2(lo[d]), B = as_h2(hi[d]);
        const float a0 = (float)A.x, a1 = (float)A.y, b0 = (float)B.x, b1 = (float)B.y;
        h2 L, H;
        L.x = (f16_t)rot_lo(a0, b0, c[2 * d], s[2 * d]);
        L.y = (f16_t)rot_lo(a1, b1, c[2 * d + 1], s[2 * d + 1]);
        H.x = (f16_t)rot_hi(a0, b0, c[2 * d], s[2 * d]);
        H.y = (f16_t)rot_hi(a1, b1, c[2 * d + 1], s[2 * d + 1]);
        lo[d] = as_u(L);
        hi[d] = as_u(H);
    }
}

// fp16 cache, head_size % 16 == 0. Units of 64 items; the first half of the units are K's, the second half V's (uniform per wave)
__global__ void __launch_bounds__(KS_T) kv_shift_f16_kernel(const ShiftArgs a) {
    const int hs = a.head_size, cph = hs >> 4;                                  // chunk pairs per head
    const long long per_which = (long long)a.n_layers * a.n_kv_heads * cph, upw = (per_which + KS_T - 1) / KS_T;
    const long long rowb = (long long)a.n_kv_heads * hs * 2;                    // bytes of a row
    for (long long u = blockIdx.x; u < 2 * upw; u += gridDim.x) {
        const bool is_v = u >= upw;
        const long long item = (is_v ? u - upw : u) * KS_T + threadIdx.x;
        if (item >= per_which) continue;
        const int j = (int)(item % cph);
        const long long lh = item / cph;
        const int head = (int)(lh % a.n_kv_heads);
        const long long layer = lh / a.n_kv_heads;
        char* col = (is_v ? a.v : a.k) + layer * a.seq_len * rowb + ((long long)head * hs + 8 * j) * 2;
        float c[8], s[8];
        if (!is_v) {
#pragma unroll
            for (int e = 0; e < 8; e++) { const float2 t = a.cs[8 * j + e]; c[e] = t.x; s[e] = t.y; }
        }
        u32x4 lo[KS_U], hi[KS_U];
#pragma unroll
        for (int i = 0; i < KS_U; i++)
            if (a.r0 + i < a.n_pos) {
                const char* src = col + (long long)(a.r0 + i) * rowb;
                lo[i] = ld16(src);
                hi[i] = ld16(src + hs);
            }
        for (int base = a.r0; base < a.n_pos; base += KS_U) {
#pragma unroll
            for (int i = 0; i < KS_U; i++) {
                const int r = base + i;
                if (r < a.n_pos) {
                    u32x4 x = lo[i], y = hi[i];
                    if (!is_v) rotate8(x, y, c, s);
                    char* dst = col + (long long)(r - a.D) * rowb;
                    st16(dst, x);
                    st16(dst + hs, y);
                    if (r + KS_U < a.n_pos) {                                   // the slot's next row: above every row stored so far
                        const char* src = col + (long long)(r + KS_U) * rowb;
                        lo[i] = ld16(src);
                        hi[i] = ld16(src + hs);
                    }
                }
            }
        }
    }
}

// fp16 cache, any even head size, any alignment: one pair of halves per item, row by row
__global__ void __launch_bounds__(256) kv_shift_f16_scalar_kernel(const ShiftArgs a) {
    const int hs = a.head_size, hp = hs >> 1;
    const long long per_which = (long long)a.n_layers * a.n_kv_heads * hp;
    const long long rowe = (long long)a.n_kv_heads * hs;                        // halves of a row
    for (long long w = (long long)blockIdx.x * blockDim.x + threadIdx.x; w < 2 * per_which; w += (long long)gridDim.x * blockDim.x) {
        const bool is_v = w >= per_which;
        const long long item = is_v ? w - per_which : w;
        const int i = (int)(item % hp);
        const long long lh = item / hp;
        const int head = (int)(lh % a.n_kv_heads);
        const long long layer = lh / a.n_kv_heads;
        uint16_t* col = reinterpret_cast<uint16_t*>(is_v ? a.v : a.k) + layer * a.seq_len * rowe + (long long)head * hs + i;
        float c = 1.f, s = 0.f;
        if (!is_v) { const float2 t = a.cs[i]; c = t.x; s = t.y; }
        for (int r = a.r0; r < a.n_pos; r++) {
            const uint16_t* src = col + (long long)r * rowe;
            uint16_t x = src[0], y = src[hp];
            if (!is_v) {
                const float fa = h2f(x), fb = h2f(y);
                x = f2h(rot_lo(fa, fb, c, s));
                y = f2h(rot_hi(fa, fb, c, s));
            }
            uint16_t* dst = col + (long long)(r - a.D) * rowe;
            dst[0] = x;
            dst[hp] = y;
        }
    }
}

// a K row's 16 bytes of this lane: dequantise (own and the pair partner's), rotate, round to half, quantise again. Every lane of the row's LPR group
// is active (shuffles); kv8_quantise's rule, restated for a row that sits in registers
template <int LPR>
__device__ __forceinline__ void rotate_requantise(u32x4& bytes, int& e, const float (&c)[16], const float (&s)[16], const bool upper) {
    u32x4 other;
#pragma unroll
    for (int d = 0; d < 4; d++) other[d] = (unsigned)__shfl_xor((int)bytes[d], LPR / 2);
    const float scale = pow2f(e);                    // byte * 2^e is exact in fp32 (and an fp16 number)
    float x[16];
#pragma unroll
    for (int d = 0; d < 4; d++) {
        const auto m0 = __builtin_amdgcn_cvt_pk_f32_fp8((int)bytes[d], false), m1 = __builtin_amdgcn_cvt_pk_f32_fp8((int)bytes[d], true);
        const auto o0 = __builtin_amdgcn_cvt_pk_f32_fp8((int)other[d], false), o1 = __builtin_amdgcn_cvt_pk_f32_fp8((int)other[d], true);
        const float m[4] = {m0[0] * scale, m0[1] * scale, m1[0] * scale, m1[1] * scale};
        const float o[4] = {o0[0] * scale, o0[1] * scale, o1[0] * scale, o1[1] * scale};
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int i = 4 * d + k;
            // lower lanes hold a and fetch b: (a * c) + (b * s); upper lanes hold b and fetch a: (b * c) - (a * s)
            const float r = upper ? rot_hi(o[k], m[k], c[i], s[i]) : rot_lo(m[k], o[k], c[i], s[i]);
            x[i] = (float)(f16_t)r;
        }
    }
    float amax = 0.f;
#pragma unroll
    for (int i = 0; i < 16; i++) amax = fmaxf(amax, fabsf(x[i]));
#pragma unroll
    for (int o = 1; o < LPR; o <<= 1) amax = fmaxf(amax, __shfl_xor(amax, o));
    e = KS_E_MIN;
    float lim = 448.f * 0x1p-15f;
    while (e < KS_E_MAX && amax > lim) { e++; lim *= 2.f; }
    const float inv = pow2f(-e);
#pragma unroll
    for (int d = 0; d < 4; d++) {
        float q[4];
#pragma unroll
        for (int k = 0; k < 4; k++) q[k] = fminf(fmaxf(x[4 * d + k] * inv, -448.f), 448.f);
        int w = 0;
        w = __builtin_amdgcn_cvt_pk_fp8_f32(q[0], q[1], w, false);
        w = __builtin_amdgcn_cvt_pk_fp8_f32(q[2], q[3], w, true);
        bytes[d] = (unsigned)w;
    }
}

// FP8 cache: an item is one lane of a head's row (16 bytes); a row's LPR lanes are neighbours inside one wave, and a group is whole or absent
template <int LPR>
__global__ void __launch_bounds__(KS_T) kv_shift_fp8_kernel(const ShiftArgs a) {
    const int hs = a.head_size;
    const long long per_which = (long long)a.n_layers * a.n_kv_heads * LPR, upw = (per_which + KS_T - 1) / KS_T;
    const long long rowb = (long long)a.n_kv_heads * hs;
    for (long long u = blockIdx.x; u < 2 * upw; u += gridDim.x) {
        const bool is_v = u >= upw;
        const long long item = (is_v ? u - upw : u) * KS_T + threadIdx.x;
        if (item >= per_which) continue;                                        // (per_which is a multiple of LPR, KS_T too: whole groups leave)
        const int sub = (int)(item % LPR);
        const long long lh = item / LPR;
        const int head = (int)(lh % a.n_kv_heads);
        const long long layer = lh / a.n_kv_heads;
        char* col = (is_v ? a.v : a.k) + layer * a.seq_len * rowb + (long long)head * hs + sub * 16;
        int8_t* ex = (is_v ? a.v_exp : a.k_exp) + (layer * a.n_kv_heads + head) * a.seq_len;
        const bool upper = sub >= LPR / 2;
        float c[16], s[16];
        if (!is_v) {
#pragma unroll
            for (int i = 0; i < 16; i++) { const float2 t = a.cs[(sub % (LPR / 2)) * 16 + i]; c[i] = t.x; s[i] = t.y; }
        }
        u32x4 q[KS_U];
        int qe[KS_U];
#pragma unroll
        for (int i = 0; i < KS_U; i++)
            if (a.r0 + i < a.n_pos) {
                q[i] = ld16(col + (long long)(a.r0 + i) * rowb);
                qe[i] = ex[a.r0 + i];
            }
        for (int base = a.r0; base < a.n_pos; base += KS_U) {
#pragma unroll
            for (int i = 0; i < KS_U; i++) {
                const int r = base + i;
                if (r < a.n_pos) {                                              // (uniform over the wave)
                    u32x4 x = q[i];
                    int e = qe[i];
                    if (!is_v) rotate_requantise<LPR>(x, e, c, s, upper);
                    st16(col + (long long)(r - a.D) * rowb, x);
                    if (sub == 0) ex[r - a.D] = (int8_t)e;
                    if (r + KS_U < a.n_pos) {
                        q[i] = ld16(col + (long long)(r + KS_U) * rowb);
                        qe[i] = ex[r + KS_U];
                    }
                }
            }
        }
    }
}

unsigned grid_for(long long units) {
    const long long room = (long long)stream_cu_count() * KS_BLOCKS_PER_CU;
    return (unsigned)(units < room ? units : room);
}

}  // namespace

namespace q4 {

int kv_shift_check(const void* k, const void* v, const int8_t* k_exp, const int8_t* v_exp, int kv_format, int n_layers, int seq_len, int n_kv_heads,
                   int head_size, int n_pos, int n_keep, int n_discard, const float* cos_sin) {
    if (!k || !v || !cos_sin || (kv_format != Q4_KV_FP16 && kv_format != Q4_KV_FP8)) return Q4_ERR_ARG;
    if (n_layers < 1 || seq_len < 1 || seq_len > Q4_MAX_SEQ_LEN || n_kv_heads < 1 || head_size < 1 || (head_size & 1) || n_pos < 1 || n_keep < 0 || n_discard < 1)
        return Q4_ERR_ARG;
    if ((long long)n_keep + n_discard > n_pos || n_pos > seq_len) return Q4_ERR_ARG;
    if (kv_format == Q4_KV_FP8) {
        if (!k_exp || !v_exp || !kv8_head_size_ok(head_size)) return Q4_ERR_ARG;
        if ((((uintptr_t)k | (uintptr_t)v) & 15) != 0) return Q4_ERR_ARG;          // rows of head_size bytes from a 16-byte aligned base
    }
    return Q4_OK;
}

int launch_kv_shift(void* k, void* v, int8_t* k_exp, int8_t* v_exp, int kv_format, int n_layers, int seq_len, int n_kv_heads, int head_size, int n_pos,
                    int n_keep, int n_discard, const float* cos_sin) {
    Q4_TRY(kv_shift_check(k, v, k_exp, v_exp, kv_format, n_layers, seq_len, n_kv_heads, head_size, n_pos, n_keep, n_discard, cos_sin));
    if (n_keep + n_discard == n_pos) return Q4_OK;                              // no row moves: a pure truncation
    const ShiftArgs a = {(char*)k, (char*)v, k_exp, v_exp, (const float2*)cos_sin, n_layers, seq_len, n_kv_heads, head_size, n_keep + n_discard, n_pos, n_discard};
    if (kv_format == Q4_KV_FP8) {
        const int lpr = head_size / 16;
        const long long units = 2 * (((long long)n_layers * n_kv_heads * lpr + KS_T - 1) / KS_T);
        const dim3 grid(grid_for(units));
        if (lpr == 4) Q4_LAUNCH(kv_shift_fp8_kernel<4>, grid, dim3(KS_T), 0, a);
        else if (lpr == 8) Q4_LAUNCH(kv_shift_fp8_kernel<8>, grid, dim3(KS_T), 0, a);
        else Q4_LAUNCH(kv_shift_fp8_kernel<16>, grid, dim3(KS_T), 0, a);
    } else if (head_size % 16 == 0 && (((uintptr_t)k | (uintptr_t)v) & 15) == 0) {
        const long long units = 2 * (((long long)n_layers * n_kv_heads * (head_size / 16) + KS_T - 1) / KS_T);
        Q4_LAUNCH(kv_shift_f16_kernel, dim3(grid_for(units)), dim3(KS_T), 0, a);
    } else {
        const long long units = (2ll * n_layers * n_kv_heads * (head_size / 2) + 255) / 256;
        Q4_LAUNCH(kv_shift_f16_scalar_kernel, dim3(grid_for(units)), dim3(256), 0, a);
    }
    Q4_LAUNCH_CHECK();
    return Q4_OK;
}

}  // namespace q4

extern "C" int q4_kv_shift(void* k, void* v, int8_t* k_exp, int8_t* v_exp, int kv_format, int n_layers, int seq_len, int n_kv_heads, int head_size, int n_pos,
                           int n_keep, int n_discard, const float* cos_sin) {
    return launch_kv_shift(k, v, k_exp, v_exp, kv_format, n_layers, seq_len, n_kv_heads, head_size, n_pos, n_keep, n_discard, cos_sin);
}
