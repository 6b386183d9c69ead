// logit_block.h -- what the single-block launches over a step's fp16 logits share (q4_logprobs.hip, q4_guide.hip, q4_dry.hip, q4_logit_process.hip,
// q4_adaptive.hip): ONE block of LB_T threads, thread t owns the 16-byte chunks t, t + LB_T, ... (8 consecutive logits each) and, past the last whole
// chunk, one tail element. The 16-bit monotone key of a half, a chunk's halves, the finish of a rewritten logit and the block-wide int reductions.
// Everything is inlined into its kernel: the header adds no symbol.
#pragma once
#include <math.h>
#include "q4_device.h"
#pragma clang fp contract(off)

namespace q4 {

constexpr int LB_T = 1024, LB_W = 16;                  // threads, waves

// monotone key of a half: larger value <=> larger key. -0 -> +0 (equal under argmax_kernel's float compare), NaN -> 0 (below -inf: never wins, like there)
static __device__ __forceinline__ unsigned half_key(unsigned h) {
    if (h == 0x8000u) h = 0u;
    if ((h & 0x7FFFu) > 0x7C00u) return 0u;
    return (h & 0x8000u) ? (~h & 0xFFFFu) : (h | 0x8000u);
}
static __device__ __forceinline__ unsigned key_half(unsigned key) { return (key & 0x8000u) ? (key & 0x7FFFu) : (~key & 0xFFFFu); }   // (key 0 -> a NaN)
// the 8 halves of a chunk, in index order
static __device__ __forceinline__ unsigned half_of(const u32x4& q, int e) { return (q[e >> 1] >> ((e & 1) * 16)) & 0xFFFFu; }
static __device__ __forceinline__ u32x4 chunk_keys(const u32x4& q) {
    u32x4 k;
#pragma unroll
    for (int d = 0; d < 4; d++) k[d] = half_key(q[d] & 0xFFFFu) | (half_key(q[d] >> 16) << 16);
    return k;
}
// half e of a chunk becomes -inf
static __device__ __forceinline__ void mask_half(u32x4& q, int e) { q[e >> 1] = (q[e >> 1] & ~(0xFFFFu << ((e & 1) * 16))) | (0xFC00u << ((e & 1) * 16)); }

// a rewritten logit: a finite value clamped to the half range and rounded (RNE); an infinity stays; a NaN is 0x7E00
static __device__ __forceinline__ q4_half finish(float v) {
    if (v != v) return (q4_half)0x7E00u;
    if (fabsf(v) != INFINITY) v = fminf(fmaxf(v, -65504.0f), 65504.0f);
    return (q4_half)f2h(v);
}

// Block-wide sum / maximum / exclusive prefix sum of one int per thread. `use` counts the calls: two LDS rows (of N >= LB_W words) take turns, so ONE
// barrier per call is enough (a row is written again only two calls later, behind the barrier of the call in between, which every thread passes after
// its reads). Every thread gets the result.
template <int N>
static __device__ __forceinline__ int block_sum(int v, int (*red)[N], int& use) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    int* row = red[use++ & 1];
    if ((threadIdx.x & 63) == 0) row[threadIdx.x >> 6] = v;
    __syncthreads();
    int s = 0;
#pragma unroll
    for (int w = 0; w < LB_W; w++) s += row[w];
    return s;
}
template <int N>
static __device__ __forceinline__ int block_max(int v, int (*red)[N], int& use) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = max(v, __shfl_xor(v, off));
    int* row = red[use++ & 1];
    if ((threadIdx.x & 63) == 0) row[threadIdx.x >> 6] = v;
    __syncthreads();
    int s = row[0];
#pragma unroll
    for (int w = 1; w < LB_W; w++) s = max(s, row[w]);
    return s;
}
template <int N>
static __device__ __forceinline__ int block_scan(int v, int (*red)[N], int& use, int& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int x = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int o = __shfl_up(x, off);
        if (lane >= off) x += o;
    }
    int* row = red[use++ & 1];
    if (lane == 63) row[wave] = x;
    __syncthreads();
    int before = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < LB_W; w++) {
        const int r = row[w];
        tot += r;
        before += w < wave ? r : 0;
    }
    total = tot;
    return before + x - v;
}

}  // namespace q4
