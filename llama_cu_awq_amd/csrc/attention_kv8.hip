// attention_kv8.hip -- the launches of attention_kv8.h: attention over the FP8 (e4m3) K / V cache, appending this position's rows.
#include <hip/hip_runtime.h>
#include <math.h>
#include "attention_kv8.h"
#include "q4_internal.h"

namespace q4 {

bool kv8_head_size_ok(int head_size) { return head_size == 64 || head_size == 128 || head_size == 256; }

// Which form the launch below takes for a bin argument (its one place; the plan of a prompt or verify pass asks too, q4_passes.hip): split-context from
// g_att_split_min up where the scratch holds the records -- 256 positions per block, or 128 for a 128-wide head up to bin 1024 (the fp16 launch's
// choice) --, else the one-pass form.
Kv8Form attention_kv8_form(int num_heads, int head_size, int max_seq_len, bool have_scratch, size_t scratch_bytes) {
    Kv8Form f;
    f.chunk = head_size == 128 && max_seq_len <= 1024 ? 128 : 256;
    f.nsp = divUp(max_seq_len, f.chunk);
    f.split = max_seq_len >= g_att_split_min && have_scratch &&
              (size_t)num_heads * f.nsp * (head_size + ATT_REC_PAD) * sizeof(float) <= scratch_bytes;
    return f;
}

// exp_stride: positions per kv head in the exponent arrays (the model's seq_len; the public entry's max_seq_len). scratch / arrive: as launch_attention
int launch_attention_kv8(q4_half* output, const q4_half* q, uint8_t* k8, uint8_t* v8, int8_t* k_exp, int8_t* v_exp, const q4_half* k_row,
                         const q4_half* v_row, int num_heads, int head_size, int kv_mul, int max_seq_len, int exp_stride, const int* pPos,
                         float* scratch, size_t scratch_bytes, unsigned* arrive) {
    if (!kv8_head_size_ok(head_size)) {
        snprintf(g_last_error, sizeof(g_last_error), "FP8 KV cache: head size %d is not supported (64, 128 or 256)", head_size);
        return Q4_ERR_UNSUPPORTED_SIZE;
    }
    if (kv_mul < 1 || num_heads % kv_mul || max_seq_len < 1 || exp_stride < 1 || !pPos) return Q4_ERR_ARG;   // (the bin may exceed a short model's seq_len: nothing at or past the position is read)
    const int kv_dim = head_size * num_heads / kv_mul;
    const float alpha = (float)(1.0 / sqrt((double)head_size));                     // llama2_q4.cu:273
    Kv8Args a = {output, q, k8, v8, k_exp, v_exp, k_row, v_row, head_size, kv_mul, kv_dim, exp_stride, pPos, alpha, max_seq_len, scratch, arrive};
    const dim3 block(ATT_NW * 64);
    const Kv8Form form = attention_kv8_form(num_heads, head_size, max_seq_len, scratch != nullptr, scratch_bytes);
    const int chunk = form.chunk, nsp = form.nsp;
    if (form.split) {
        const size_t smem = (size_t)(32 + ATT_NW * head_size) * 4;
        const dim3 grid(num_heads, nsp);
        if (head_size == 64) Q4_LAUNCH((attention_kv8_split_kernel<4, 1>), grid, block, smem, a);          // 16 waves x 16 rows
        else if (head_size == 256) Q4_LAUNCH((attention_kv8_split_kernel<16, 4>), grid, block, smem, a);   // 16 x 4 x 4
        else if (chunk == 128) Q4_LAUNCH((attention_kv8_split_kernel<8, 1>), grid, block, smem, a);        // 16 x 8
        else Q4_LAUNCH((attention_kv8_split_kernel<8, 2>), grid, block, smem, a);
        if (arrive == nullptr)
            Q4_LAUNCH(attention_combine_kernel, dim3(num_heads), dim3(128), 0, output, (const float*)scratch, head_size, nsp);
        Q4_LAUNCH_CHECK();
        return Q4_OK;
    }
    const size_t smem = (size_t)(32 + ATT_NW * head_size + max_seq_len) * 4;
    if (smem > 160 * 1024) return Q4_ERR_UNSUPPORTED_SIZE;
    const dim3 grid(num_heads);
#define Q4_KV8(L)                                                                                          \
    {                                                                                                      \
        { const int rc = lds_opt_in((const void*)attention_kv8_kernel<L>, smem); if (rc) return rc; }      \
        Q4_LAUNCH((attention_kv8_kernel<L>), grid, block, smem, a);                                        \
    }
    if (head_size == 64) Q4_KV8(4) else if (head_size == 128) Q4_KV8(8) else Q4_KV8(16)
#undef Q4_KV8
    Q4_LAUNCH_CHECK();
    return Q4_OK;
}

}  // namespace q4

using namespace q4;

// MultiHeadAttention over caller-owned FP8 caches: k8 / v8 [max_seq_len][kv_dim] e4m3 bytes, k_exp / v_exp [n_kv_heads][max_seq_len] int8, k_row / v_row
// [kv_dim] halves holding position *pPos (K rotated), which the launch quantises, uses and appends. `att`: null, or the caller's scratch for the
// split-context records, 8 bytes per (head, position) -- q4_multi_head_attention's n_heads * max_seq_len halves hold them for 64-wide heads only.
extern "C" int q4_multi_head_attention_kv8(q4_half* output, const q4_half* q, uint8_t* k8, uint8_t* v8, int8_t* k_exp, int8_t* v_exp,
                                           const q4_half* k_row, const q4_half* v_row, q4_half* att, int num_heads, int head_size, int kv_mul,
                                           int max_seq_len, const int* pPos) {
    if (!output || !q || !k8 || !v8 || !k_exp || !v_exp || !k_row || !v_row) return Q4_ERR_ARG;
    const size_t att_bytes = att ? (size_t)num_heads * max_seq_len * 8 : 0;
    return launch_attention_kv8(output, q, k8, v8, k_exp, v_exp, k_row, v_row, num_heads, head_size, kv_mul, max_seq_len, max_seq_len, pPos,
                                (float*)att, att_bytes, nullptr);
}
