// prompt_pass_kv8.h -- the K / V side of a prompt or verify pass of a model with the FP8 (e4m3) cache (q4_set_pass_kv8; prompt_pass_kv8.hip, DESIGN.md
// section 3.7 "FP8 cache"). The pass's q/k/v launch leaves the tokens' K (rotated) and V as fp16 in staging rows [PROMPT_PASS_MAX][kv_dim]; ONE append
// launch per layer quantises them into the byte caches exactly as the step's attention launch appends its row; the attention launch behind it reads every
// row, the tokens' own included, from the cache -- the bytes and exponents the step holds in registers for its current row (attention_kv8.h).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "q4_internal.h"

namespace q4 {

// What the layer's launches of an FP8 pass share: the caches and exponent arrays already offset to the layer, exp_stride positions per kv head
struct PassKv8 {
    uint8_t* k8;
    uint8_t* v8;
    int8_t* k_exp;
    int8_t* v_exp;
    int n_heads, head_size, kv_mul, kv_dim, exp_stride;
    const int* pos;              // [ntok] the tokens' positions, ascending by one (device)
    int ntok;
};
// rows pos[t] of both caches and both exponent arrays from the staging rows k_rows / v_rows [ntok][kv_dim]
int launch_pass_kv8_append(const PassKv8& c, const q4_half* k_rows, const q4_half* v_rows);
// the one-pass form (every position's bin argument <= 256): xb[t] = attention of q[t] over rows [0, pos[t]]; xb / q rows `dim` halves apart
int launch_pass_kv8_attention(const PassKv8& c, q4_half* xb, const q4_half* q, int dim, float alpha);
// the split-context form, chunk 128 or 256: token t's flash-decode records into records + t * tok_stride, [n_heads][nsp][head_size + ATT_REC_PAD] floats
// (prompt_merge_kernel merges them)
int launch_pass_kv8_split(const PassKv8& c, float* records, size_t tok_stride, const q4_half* q, int dim, float alpha, int chunk, int nsp);

}  // namespace q4
