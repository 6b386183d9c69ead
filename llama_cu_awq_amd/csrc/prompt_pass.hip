// prompt_pass.hip -- a prompt pass (prompt_pass.h): n consecutive prompt-only positions run layer by layer, every launch reading its
// weights ONCE into registers and looping over the n tokens' activations. Five launches per layer -- rmsnorm + q/k/v + RoPE + K/V write, attention (one
// block per (token, head, V slice); in the split-context bins, positions >= 256 under q4_set_pass_context: one block per (head, chunk) that loops over the
// tokens, and a launch that merges each token's records), o-proj + residual, rmsnorm + gate/up + SiLU, down projection + residual -- between an embedding launch and one that
// leaves RunState::x and the position words as the per-token steps would. No launch waits for another block: every dependency is a launch boundary.
// With log-probability records on (q4_set_pass_logprobs): the verify pass's classifier over the n rows and the row form of the record launch in front of
// that last launch (run_prompt_pass).
// Grouped-query models of Mistral-7B's / Llama-3-8B's shape (q4_set_pass_gqa; DESIGN.md 3.7 "Grouped-query shapes"): the q/k/v launch with per-matrix
// widths (GQA), both attention launches with kv_mul query heads per K / V head, the down projection in the step's shared-half-slot form (HALF).
// Models with the FP8 K / V cache (q4_set_pass_kv8; DESIGN.md 3.7 "FP8 cache"): the q/k/v launch leaves K / V in fp16 staging rows (STAGE), one launch
// appends them to the byte caches and attention reads every row from there (prompt_pass_kv8.hip) -- six launches per layer, seven in the split bins.
// Llama-2-13B's shape (q4_set_pass_13b; DESIGN.md 3.7 "13B"): K = dim = 5120 is two whole k-slots and the step's shared half slot (HALF without a K
// split) in the q/k/v, o-proj and gate/up launches -- a column pair per wave in the latter two --, the norm over 640 chunk partials and 128 zeros, the
// down projection in the K split's shared-half-slot form as for the grouped-query shape.
// A batch pass (q4_batch.h): the rows are the current positions of DIFFERENT sequences -- the q/k/v launch and the attention launches in their
// row forms (ROWS: a row's position and cache from per-row tables; a launch names the rows it runs), o-proj / gate-up / down as above (batch_pass_layers).
//
// The arithmetic is the per-token path's, bit for bit: a column's value in the int4 GEMV family is fixed by the staging (q4_stage_chunk on units negated by
// parity), the per-lane chain over its k-slots in slot order (fma(scale, q4_dot_unit, c)), reduce4_q4 (a row's total depends on that row's input alone) and
// the epilogue -- not by which kernel, block shape or neighbour columns compute it (gemv_q4.h; the strips, the sixteen-wave o-proj role and the three-phase
// FFN launch rest on the same fact). The body below is gemv_q4_body's steps with a token loop around steps 3 - 5, the tokens staged in groups; the attention blocks call attention_body
// with the template arguments of attention_oproj16_kernel<5 | 6>.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <math.h>
#include "layer_attn.h"
#include "prompt_pass.h"
#include "prompt_pass_kv8.h"
#include "spec_verify.h"

namespace q4 {

constexpr int PP_WAVES = 16;           // waves per block: four per SIMD hide each other's issue latency (a wave alone issues a VALU instruction every ~5 cycles)
#ifndef Q4_PP_QKV_GQA_WAVES            // (make exp EXPFLAGS=-DQ4_PP_QKV_GQA_WAVES=12: the other grid, for tools/bench_pass_gqa.py --variant-libs)
#define Q4_PP_QKV_GQA_WAVES 6
#endif
#ifndef Q4_PP_DOWN_HALF_G              // (... -DQ4_PP_DOWN_HALF_G=2: two staged tokens per group behind an LDS opt-in)
#define Q4_PP_DOWN_HALF_G 1
#endif
constexpr int PP_QKV_GQA_WAVES = Q4_PP_QKV_GQA_WAVES;    // grouped-query q/k/v (kv_dim = dim / 4): 1024 + 2 x 256 column groups = 256 blocks of six waves, one per CU (twelve-wave blocks: 128, half of the CUs idle -- a 250-token ingest 169.9 ms against 165.3)
constexpr int PP_DOWN_HALF_G = Q4_PP_DOWN_HALF_G;      // tokens staged per group by the shared-half-slot down launch: nine LDS rows of 64 units (39 KB) per token, two exceed 64 KB (behind an opt-in they measured 0.45 % faster over an ingest: not taken)
constexpr int PP_QKV_WAVES = 12;       // q/k/v: 3 x 1024 column groups = 256 blocks of twelve waves, one per CU (sixteen-wave blocks: 192, a quarter of the CUs idle)
// dim 5120 (q4_set_pass_13b): every K = 5120 launch stages three 64-unit rows per token, so a normalising launch holds three tokens per group (four are
// 16 bytes over the 64 KB that need no opt-in)
#ifndef Q4_PP_FFN13_WAVES              // (make exp EXPFLAGS=-DQ4_PP_FFN13_WAVES=9: the other grid of gate/up at N = 13824, for tools/bench_pass_13b.py --variant-libs)
#define Q4_PP_FFN13_WAVES 12
#endif
constexpr int PP13_G = 3;              // tokens per group of the normalising gate/up launch
constexpr int PP13_QKV_G = 2;          // ... of q/k/v, whose wave holds ten weight registers of four columns: three tokens spill 8 bytes at 168 registers
constexpr int PP13_QKV_WAVES = 12;     // q/k/v: 3 x 1280 column groups = 320 blocks of twelve waves (fifteen-wave blocks, one per CU, are held to 128 registers and spill 164 bytes)
constexpr int PP13_O_WAVES = 10;       // o-proj: 2560 column pairs = 256 blocks of ten waves, one per CU
constexpr int PP13_FFN_WAVES = Q4_PP_FFN13_WAVES;   // gate/up: 6912 column pairs = 576 blocks of twelve waves, one resident per CU at 138 registers -- a 250-token ingest 314.1 ms against 318.7 with 768 blocks of nine waves (three per CU, 158 registers: also one resident), byte-equal; sixteen-wave blocks are held to 128 registers and spill

// One wave owns COLS columns (KS = 2: one of the two k-parts of them); W / ZW / SC stay in registers while the tokens pass. Token t reads x + t * K and
// writes out + t * N (q/k/v: q + t * N, cache rows p0 + t), p0 = *pPos -- the device position, which no launch of the pass but the last one moves.
template <int SLOTS, int KS, bool NORM, int G>
constexpr size_t prompt_gemv_lds() {      // G tokens' permuted x and x-only sums, their norm partials, the K split's exchange slots
    using L = LdsLayout<SLOTS, KS>;
    return (size_t)G * (L::XS + L::SX + (NORM ? (size_t)L::NUNITS * 4 : 0)) + 1024 + 16;
}
// GQA (q/k/v): k and v have a.N_kv < a.N columns each; the three matrices' column groups are still dealt as one range, N / 4 groups of q and then
// N_kv / 4 of k and of v, every matrix with its own width in the descriptors, the clamp and the row addressing.
// HALF: gemv_q4_body's shared half slot -- the last slot (of a k-part: plain, K split; of the column: K = 5120, any mode) holds at most 32 units, lanes
// 0 - 31 take it for the even column of each of the wave's pairs (c, c + 1) and lanes 32 - 63 for the odd one, its term is added as a product and a sum
// and the other half of the wave adds 0.f. The pairs are the step's: q/k/v (col[0], col[1]) and (col[2], col[3]) -- the two first and the two second
// halves of two adjacent RoPE pairs, columns i, i + 1 of a head --, o-proj and gate/up columns 2 wg and 2 wg + 1 of one matrix (an even column's terms
// in lanes 0 - 31 in every step kernel: gemv_q4_body, attention_oproj16_kernel's o-proj role, both strips kernels).
// STAGE (q/k/v of a model with the FP8 cache, GemvArgs::kv_stage): out[1] / out[2] are the pass's fp16 staging rows [ntok][N] -- token t's K / V row goes
// to row t, not into a cache at loff + pos * N (prompt_pass_kv8.h appends them). A template flag: the fp16 instantiations are the code they were.
// ROWS (q/k/v of a batch pass, q4_batch.h: the rows belong to different sequences): row t sits at position a.pPos[t] -- its rotation-table row and its
// cache row -- instead of *a.pPos + t, and its K / V row goes into the cache a.row_kv[t] (K) / a.row_kv[PROMPT_PASS_MAX + t] (V) at loff + pos * N.
// Which rotation and which address a row gets is all that changes: its sums are the ones above. A template flag again.
template <int MODE, int SLOTS, int COLS, bool NORM, int KS, int G, int NW, bool GQA = false, bool HALF = false, bool STAGE = false, bool ROWS = false>
__global__ void __launch_bounds__(NW * 64) prompt_gemv_kernel(const GemvArgs a, const int ntok) {
    constexpr int NMAT = ModeTraits<MODE>::NMAT;
    static_assert(!ROWS || (MODE == MODE_QKV && !STAGE), "per-row positions and caches: q/k/v into fp16 caches");
    static_assert(!GQA || MODE == MODE_QKV, "per-matrix widths: q/k/v");
    static_assert(!STAGE || MODE == MODE_QKV, "staging rows: q/k/v");
    static_assert(!HALF || (COLS % 2 == 0 && (KS == 1 || (MODE == MODE_PLAIN && COLS == 2))), "shared half slot: column pairs; with the K split one pair per wave");
    static_assert(G >= 1 && G <= 8, "exchange slots");
    static_assert(KS == 1 || (KS == 2 && MODE == MODE_PLAIN && !NORM), "K split: plain GEMV");
    static_assert(COLS >= 1 && COLS <= 4 && (MODE != MODE_QKV || COLS == 4), "one reduce4_q4 row per column; q/k/v: two RoPE pairs per wave");
    using Lds = LdsLayout<SLOTS, KS>;
    constexpr int TS = Lds::ROWS;
    constexpr int NUNITS = Lds::NUNITS;
    constexpr int NI = (NUNITS + NW * 64 - 1) / (NW * 64);   // staging steps of the block
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    u32x4* xs = reinterpret_cast<u32x4*>(smem);                                   // [G][TS][4][64] permuted x
    float* sx = reinterpret_cast<float*>(smem + G * Lds::XS);                     // [G][TS][64]
    float* part = reinterpret_cast<float*>(smem + G * (Lds::XS + Lds::SX));       // [G][NUNITS] norm partials, or [G][NW][4] k-part totals

    const unsigned tid = threadIdx.x;
    const unsigned lane = tid & 63u;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    constexpr int nw = NW;
    // q/k/v: the three matrices' column groups are dealt as one range (N / 4 groups each), so the grid divides by any block width
    const int gidx = blockIdx.x * (nw / KS) + wave / KS;
    const int gpm = MODE == MODE_QKV ? a.N / COLS : 1;       // column groups per matrix
    const int gkv = GQA ? a.N_kv / COLS : gpm;               // ... of k and of v
    const int mat_g = gidx < gpm ? 0 : 1 + (gidx - gpm) / gkv;   // (a wave past the last group -- the host launches none -- lands on v past its columns: clamped loads, no store)
    const int mat0 = MODE == MODE_QKV ? __builtin_amdgcn_readfirstlane(GQA ? (mat_g < 2 ? mat_g : 2) : gidx / gpm) : 0;
    const int wg = MODE == MODE_QKV ? (GQA ? (mat0 == 0 ? gidx : gidx - gpm - (mat0 - 1) * gkv) : gidx - mat0 * gpm) : gidx;
    const int khalf = wave % KS;
    const unsigned ubase = KS > 1 ? (unsigned)(khalf * a.ku) : 0u;
    const unsigned uend = KS > 1 ? (ubase + (unsigned)a.ku < (unsigned)a.pw4 ? ubase + (unsigned)a.ku : (unsigned)a.pw4) : (unsigned)a.pw4;
    const unsigned nchunks = (unsigned)a.K >> 3;
    const int N = GQA && mat0 != 0 ? a.N_kv : a.N;

    int col[COLS];
    if (MODE == MODE_QKV) {
        constexpr int P = COLS / 2;
        const int hp = a.head_size >> 1;
#pragma unroll
        for (int pi = 0; pi < P; pi++) {
            const int p = wg * P + pi;
            const int head = p / hp, i = p - head * hp;
            col[pi] = head * a.head_size + i;
            col[P + pi] = col[pi] + hp;
        }
    } else {
#pragma unroll
        for (int c = 0; c < COLS; c++) col[c] = wg * COLS + c;
    }
    int colc[COLS];
#pragma unroll
    for (int c = 0; c < COLS; c++) colc[c] = col[c] < N ? col[c] : N - 1;

    int p0 = 0;
    if (MODE == MODE_QKV && !ROWS) p0 = *a.pPos;

    // ---- the first activations, the norm weights, then every weight / zero / scale of the wave (gemv_q4_body's loads: clamped, bounded descriptors).
    // A normalising kernel (K = 4096: one chunk per thread) holds a whole group's chunks; the others hold one token's and fetch the next while they stage.
    u32x4 xg[NORM ? G : 1][NI], wraw[NI];
    auto load_x = [&](int t, u32x4 (&xr)[NI]) {
        const int tc = t < ntok ? t : ntok - 1;             // past the pass's last token: the last one again (a load nobody stages)
        const u32x4* xt = reinterpret_cast<const u32x4*>(a.x + (size_t)tc * a.K);
#pragma unroll
        for (int i = 0; i < NI; i++) {
            const unsigned u = tid + i * (NW * 64);
            xr[i] = xt[u < nchunks ? u : nchunks - 1];
        }
    };
    if (NORM) {
#pragma unroll
        for (int g = 0; g < G; g++) load_x(g, xg[NORM ? g : 0]);
#pragma unroll
        for (int i = 0; i < NI; i++) {
            const unsigned u = tid + i * (NW * 64);
            wraw[i] = reinterpret_cast<const u32x4*>(a.rms_w)[u < nchunks ? u : nchunks - 1];
        }
    } else {
        load_x(0, xg[0]);
    }
    u32x4 W[NMAT][SLOTS][COLS];
    unsigned ZW[NMAT][SLOTS][COLS];
    uint16_t SC[NMAT][SLOTS][COLS];
    __amdgpu_buffer_rsrc_t rw[NMAT], rz[NMAT], rs[NMAT];
#pragma unroll
    for (int m = 0; m < NMAT; m++) {
        const GemvMat& M = a.m[mat0 + m];
        rw[m] = __builtin_amdgcn_make_buffer_rsrc((void*)M.w, 0, N * a.pw4 * 16, 0x00020000);
        rz[m] = __builtin_amdgcn_make_buffer_rsrc((void*)M.z, 0, N * a.pzh * 4, 0x00020000);
        rs[m] = __builtin_amdgcn_make_buffer_rsrc((void*)M.s, 0, N * a.sh * 2, 0x00020000);
    }
    const bool upper = lane >= 32u;
#pragma unroll
    for (int s = 0; s < SLOTS; s++) {
        if (HALF && s == SLOTS - 1) {                        // the shared half slot: the column offset per lane, kept in each pair's first entries
            const unsigned jh = ubase + s * 64 + (lane & 31u);
            const unsigned jj = jh < uend ? jh : uend - 1;
            if constexpr (KS == 2) {                         // (one pair, one matrix: the statements the K split's instantiation was compiled from)
                const unsigned cw = upper ? (unsigned)colc[COLS - 1] : (unsigned)colc[0];
                ZW[0][s][0] = __builtin_amdgcn_raw_buffer_load_b32(rz[0], (jj >> 5) * 4 + cw * a.pzh * 4, 0, Q4_ZS_AUX);
                SC[0][s][0] = __builtin_amdgcn_raw_buffer_load_b16(rs[0], (jj >> 2) * 2 + cw * a.sh * 2, 0, Q4_ZS_AUX);
                W[0][s][0] = __builtin_amdgcn_raw_buffer_load_b128(rw[0], jj * 16 + cw * a.pw4 * 16, 0, Q4_W_AUX);
            } else {
#pragma unroll
                for (int m = 0; m < NMAT; m++)
#pragma unroll
                    for (int c = 0; c < COLS; c += 2) {
                        const unsigned cw = upper ? (unsigned)colc[c + 1] : (unsigned)colc[c];
                        ZW[m][s][c] = __builtin_amdgcn_raw_buffer_load_b32(rz[m], (jj >> 5) * 4 + cw * a.pzh * 4, 0, Q4_ZS_AUX);
                        SC[m][s][c] = __builtin_amdgcn_raw_buffer_load_b16(rs[m], (jj >> 2) * 2 + cw * a.sh * 2, 0, Q4_ZS_AUX);
                        W[m][s][c] = __builtin_amdgcn_raw_buffer_load_b128(rw[m], jj * 16 + cw * a.pw4 * 16, 0, Q4_W_AUX);
                    }
            }
            continue;
        }
        const unsigned j = ubase + s * 64 + lane;
        const unsigned jj = j < uend ? j : uend - 1;        // tail lanes re-read the part's last unit
#pragma unroll
        for (int m = 0; m < NMAT; m++)
#pragma unroll
            for (int c = 0; c < COLS; c++) {
                ZW[m][s][c] = __builtin_amdgcn_raw_buffer_load_b32(rz[m], (jj >> 5) * 4, colc[c] * a.pzh * 4, Q4_ZS_AUX);
                SC[m][s][c] = __builtin_amdgcn_raw_buffer_load_b16(rs[m], (jj >> 2) * 2, colc[c] * a.sh * 2, Q4_ZS_AUX);
                W[m][s][c] = __builtin_amdgcn_raw_buffer_load_b128(rw[m], jj * 16, colc[c] * a.pw4 * 16, Q4_W_AUX);
            }
    }

    const int row = lane >> 4;
    const bool writer = (lane & 15u) == 0;
    int qkv_n = 0, qkv_i = 0;                                // q/k/v: this row's output column and its pair's index inside the head
    if (MODE == MODE_QKV) {
        const int hp = a.head_size >> 1;
        const int p = wg * 2 + (row & 1);
        const int head = p / hp;
        qkv_i = p - head * hp;
        qkv_n = head * a.head_size + qkv_i + ((row & 2) ? hp : 0);
    }

    // Tokens go through in groups of G: the group's vectors are staged side by side in LDS behind ONE pair of barriers (a token's own chain of load, norm,
    // stage and barriers costs more than its dot products), then each is consumed against the registers. Every token's arithmetic is its own.
    for (int t0 = 0; t0 < ntok; t0 += G) {
        const int ng = ntok - t0 < G ? ntok - t0 : G;
        if (t0 > 0) __syncthreads();                         // the previous group's readers of xs / sx / part are done
        // ---- 3. stage the group's x (gemv_q4_body's stage_tail per token)
        const unsigned sgn = q4_stage_sign_bits(tid);
        if constexpr (NORM) {
#pragma unroll
            for (int g = 0; g < G; g++)
                if (g < ng) {
#pragma unroll
                    for (int i = 0; i < NI; i++) {
                        const unsigned u = tid + i * (NW * 64);
                        if (u < NUNITS) part[g * NUNITS + u] = u < nchunks ? sumsq8(xg[g][i], 0.f) : 0.f;
                    }
                }
            __syncthreads();
#pragma unroll
            for (int g = 0; g < G; g++)
                if (g < ng) {
                    const float ss = q4_signed_scale(rms_scale_from_partials<NUNITS>(part + g * NUNITS, NUNITS, a.K), sgn);
#pragma unroll
                    for (int i = 0; i < NI; i++) {
                        const unsigned u = tid + i * (NW * 64);
                        u32x4 v = rms_apply8(xg[g][i], wraw[i], ss);
                        if (u >= nchunks) v = (u32x4){0u, 0u, 0u, 0u};
                        q4_stage_chunk(xs + g * NUNITS, sx + g * (TS * 64), u, v, NUNITS);
                    }
                }
        } else {
#pragma unroll
            for (int g = 0; g < G; g++)
                if (g < ng) {
                    u32x4 xn[NI];
                    load_x(t0 + g + 1, xn);                  // the next token's x travels while this one is staged
#pragma unroll
                    for (int i = 0; i < NI; i++) {
                        const unsigned u = tid + i * (NW * 64);
                        u32x4 v = q4_signed_x(xg[0][i], sgn);
                        if (u >= nchunks) v = (u32x4){0u, 0u, 0u, 0u};
                        q4_stage_chunk(xs + g * NUNITS, sx + g * (TS * 64), u, v, NUNITS);
                    }
#pragma unroll
                    for (int i = 0; i < NI; i++) xg[0][i] = xn[i];
                }
        }
        __syncthreads();
        if constexpr (NORM) {
            if (t0 + G < ntok) {                             // the next group's x travels while this one multiplies
#pragma unroll
                for (int g = 0; g < G; g++) load_x(t0 + G + g, xg[NORM ? g : 0]);
            }
        }

        // what the group's epilogues read from memory, requested in front of its dot products (read in the epilogue, each is a dependent round trip per
        // token): the residual of the lane's output (this lane is its only writer), the rotation of its pair
        const int n_out = MODE == MODE_QKV ? qkv_n : wg * COLS + row;
        const bool out_lane = writer && (MODE == MODE_QKV || row < COLS) && (KS == 1 || khalf == 0) && n_out < N;
        uint16_t resid[G];
        float2 rot[G];
        int posr[ROWS ? G : 1];                              // ROWS: the group's positions
#pragma unroll
        for (int g = 0; g < G; g++) {
            resid[g] = 0;
            rot[g] = float2{1.f, 0.f};
            if constexpr (ROWS) posr[g] = a.pPos[g < ng ? t0 + g : t0];
            if (g < ng) {
                if (MODE == MODE_PLAIN && a.accum && out_lane) resid[g] = a.out[0][(size_t)(t0 + g) * N + n_out];
                if constexpr (ROWS) {
                    if (mat0 < 2) rot[g] = a.rope_table[(size_t)posr[g] * (a.head_size >> 1) + qkv_i];
                } else {
                    if (MODE == MODE_QKV && mat0 < 2) rot[g] = a.rope_table[(size_t)(p0 + t0 + g) * (a.head_size >> 1) + qkv_i];
                }
            }
        }

#pragma unroll
        for (int g = 0; g < G; g++) {
            if (g >= ng) break;
            const int t = t0 + g;
            const u32x4* xst = xs + g * NUNITS;
            const float* sxt = sx + g * (TS * 64);
            // the nibble masks are taken again for every token (q4_dot_unit): kept across the token loop they are four registers per weight register
#pragma unroll
            for (int m = 0; m < NMAT; m++)
#pragma unroll
                for (int s = 0; s < SLOTS; s++)
#pragma unroll
                    for (int c = 0; c < COLS; c++)
                        if (!(HALF && s == SLOTS - 1 && (c & 1))) asm volatile("" : "+v"(W[m][s][c]));
            // ---- 4. consume in slot order
            float colsum[NMAT][4];
#pragma unroll
            for (int m = 0; m < NMAT; m++)
#pragma unroll
                for (int c = 0; c < 4; c++) colsum[m][c] = 0.f;
#pragma unroll
            for (int s = 0; s < SLOTS; s++) {
                const bool hs = HALF && s == SLOTS - 1;      // both halves of the wave read the slot's units 0 - 31
                const unsigned lu = hs ? (lane & 31u) : lane;
                unsigned j = ubase + s * 64 + lu;
                unsigned jx = j;
                if (KS > 1) {                                // past the part's end: the all-zero row
                    jx = j < uend ? j : (unsigned)((TS - 1) * 64);
                    j = j < uend ? j : uend - 1;
                }
                u32x4 X[4];
                const unsigned xrow = KS > 1 ? ((jx >> 6) << 8) + (jx & 63u) : (unsigned)((s * 4) << 6) + lu;
#pragma unroll
                for (int d = 0; d < 4; d++) X[d] = xst[xrow + (d << 6)];
                const float corr = sxt[KS > 1 ? jx : (unsigned)(s * 64) + lu];
                const unsigned zsh = ((j >> 2) & 7u) * 4u;
                if (hs) {                                    // gemv_q4_body's half slot, word for word: lanes 0 - 31 worked for column c, lanes 32 - 63 for column c + 1
                    if constexpr (KS == 2) {
                        const float tt = q4_dot_unit(W[0][s][0], X, ZW[0][s][0], zsh, corr);
                        const float v = h2f(SC[0][s][0]) * tt;
                        colsum[0][0] += upper ? 0.f : v;
                        colsum[0][COLS - 1] += upper ? v : 0.f;
                    } else {
#pragma unroll
                        for (int m = 0; m < NMAT; m++)
#pragma unroll
                            for (int c = 0; c < COLS; c += 2) {
                                const float tt = q4_dot_unit(W[m][s][c], X, ZW[m][s][c], zsh, corr);
                                const float v = h2f(SC[m][s][c]) * tt;
                                colsum[m][c] += upper ? 0.f : v;
                                colsum[m][c + 1] += upper ? v : 0.f;
                            }
                    }
                    continue;
                }
#pragma unroll
                for (int m = 0; m < NMAT; m++)
#pragma unroll
                    for (int c = 0; c < COLS; c++) {
                        const float tt = q4_dot_unit(W[m][s][c], X, ZW[m][s][c], zsh, corr);
                        colsum[m][c] = __builtin_fmaf(h2f(SC[m][s][c]), tt, colsum[m][c]);
                    }
            }

            // ---- 5. reduction (row r: the wave's column r; rows past COLS reduce zeros) + epilogue
            if constexpr (MODE == MODE_PLAIN) {
                float tot = reduce4_q4(colsum[0][0], colsum[0][1], colsum[0][2], colsum[0][3]) * 1048576.f;
                if (KS > 1) {                                // fixed order: k-parts from the lowest up (a slot of its own per token of the group)
                    float* ex = part + g * (NW * 4);
                    if (writer) ex[wave * 4 + row] = tot;
                    __syncthreads();
                    if (khalf == 0) tot += ex[(wave + 1) * 4 + row];
                }
                if (out_lane) {
                    float r = tot;
                    if (a.accum) r += h2f(resid[g]);
                    a.out[0][(size_t)t * N + n_out] = f2h(r);
                }
            } else if constexpr (MODE == MODE_FFN) {         // gate in gg and up in uu
                const float gg = reduce4_q4(colsum[0][0], colsum[0][1], colsum[0][2], colsum[0][3]) * 1048576.f;
                const float uu = reduce4_q4(colsum[NMAT - 1][0], colsum[NMAT - 1][1], colsum[NMAT - 1][2], colsum[NMAT - 1][3]) * 1048576.f;
                float val = gg;
                val *= 1.0f / (1.0f + expf(-val));           // gpu_kernels.h:271
                val *= uu;                                   // :272
                if (out_lane) a.out[0][(size_t)t * N + n_out] = f2h(val);
            } else {                                         // MODE_QKV: rows = pair0 first, pair1 first, pair0 second, pair1 second
                const int pos = ROWS ? posr[ROWS ? g : 0] : p0 + t;
                q4_half* out = mat0 == 0 ? a.out[0] + (size_t)t * N : a.out[mat0] + (size_t)a.loff + (size_t)pos * N;
                if constexpr (STAGE) {
                    if (mat0 != 0) out = a.out[mat0] + (size_t)t * N;
                }
                if constexpr (ROWS) {
                    if (mat0 != 0) out = a.row_kv[(mat0 - 1) * PROMPT_PASS_MAX + t] + (size_t)a.loff + (size_t)pos * N;
                }
                const float mine = reduce4_q4(colsum[0][0], colsum[0][1], colsum[0][2], colsum[0][3]) * 1048576.f;
                float r = mine;
                if (mat0 < 2) {
                    const float other = round_h(__shfl_xor(mine, 32));
                    const float me = round_h(mine);
                    const float fcr = rot[g].x, fci = rot[g].y;
                    r = (row & 2) ? (other * fci + me * fcr) : (me * fcr - other * fci);    // gpu_kernels.h:345-346
                }
                if (out_lane) out[n_out] = f2h(r);
            }
        }
    }
}

// Attention of the pass: block b of token t is unit b of attention_oproj16_kernel's attention role at position p0 + t -- the rows up to it were written by
// the launch in front. The role's granules go to a sink of the pass's own with tag 0 (no launch's tag); what counts is the plain copy in xb[t].
__global__ void __launch_bounds__(LA16_WAVES * 64) prompt_attention_kernel(const AttArgs a0, const int* pos_arr, u32x2v* sink, const unsigned sink_stride,
                                                                           const unsigned nheads, const unsigned natt, const int dim) {
    const unsigned t = blockIdx.x / natt, b = blockIdx.x % natt;
    AttArgs a = a0;
    a.pPos = pos_arr + t;
    a.q = a0.q + (size_t)t * dim;
    a.output = a0.output + (size_t)t * dim;
    Handoff ho = {};
    ho.pub = sink + (size_t)t * sink_stride;
    const int pos = __builtin_amdgcn_readfirstlane(pos_arr[t]);
    if (pos < 128) {
        a.lds_scores = 128;
        attention_body<16, 2, LA16_WAVES, 2, false, 4, 0, 8>(a, (int)(b % nheads), ho, (int)(b / nheads));
    } else {
        a.lds_scores = 256;
        attention_body<16, 4, LA16_WAVES, 2, false, 4, 128, 8>(a, (int)(b % nheads), ho, (int)(b / nheads));
    }
}

// The row form for a batch pass (q4_batch.h): the rows of one pass belong to different sequences, so a launch names the rows it runs (the ones whose
// step takes this attention form) and every row reads its own cache -- kv[row] (K) / kv[PROMPT_PASS_MAX + row] (V) plus the layer's offset. Block b of
// listed row i is prompt_attention_kernel's block b of token t = list.row[i]: the same unit at the same position over that sequence's rows.
__global__ void __launch_bounds__(LA16_WAVES * 64) prompt_attention_rows_kernel(const AttArgs a0, const int* pos_arr, u32x2v* sink, const unsigned sink_stride,
                                                                                const unsigned nheads, const unsigned natt, const int dim, const PassRowList list,
                                                                                q4_half* const* kv, const long long loff) {
    const unsigned t = (unsigned)list.row[blockIdx.x / natt], b = blockIdx.x % natt;
    AttArgs a = a0;
    a.pPos = pos_arr + t;
    a.q = a0.q + (size_t)t * dim;
    a.output = a0.output + (size_t)t * dim;
    a.key_cache = kv[t] + loff;
    a.value_cache = kv[PROMPT_PASS_MAX + t] + loff;
    Handoff ho = {};
    ho.pub = sink + (size_t)t * sink_stride;
    const int pos = __builtin_amdgcn_readfirstlane(pos_arr[t]);
    if (pos < 128) {
        a.lds_scores = 128;
        attention_body<16, 2, LA16_WAVES, 2, false, 4, 0, 8>(a, (int)(b % nheads), ho, (int)(b / nheads));
    } else {
        a.lds_scores = 256;
        attention_body<16, 4, LA16_WAVES, 2, false, 4, 128, 8>(a, (int)(b % nheads), ho, (int)(b / nheads));
    }
}

// Attention of a pass whose tokens sit in the split-context bins (positions >= 256 where the step runs forms 4 / 2 / 3 inside attention_oproj_kernel:
// one block of LA_WAVES waves per (head, chunk of 64 / 128 / 256 positions), a flash-decode record per chunk, the records merged in chunk order). Block
// (h, sp) requests the chunk's K and V rows ONCE -- split_live's request order and policy, clamped to the last row the pass may read -- and loops over the
// pass's tokens: each token's record is split_live's middle restated on the same helpers (row_sum<16>, round_h, wave_max / row16_max, expf, the fma chain
// over u in order, the shuffle folds, wave_sum / row16_sum, split_store_record<false, LA_WAVES>) with size = pos[t] + 1, written to token t's own record
// area as plain floats. A record depends on the chunk's rows, q, size and the reduction shape -- not on whether it leaves as granules or floats -- so the
// words are the step's. No tag, no poll, no counter, no atomic: the merge is the next launch (prompt_merge_kernel).
//  * rows above a token's position are later tokens' rows (or stale ones), possibly non-finite: a masked lane multiplies its zero probability by the V
//    row the step's clamp would have handed it -- row pos[t], the token's own -- never by the row it holds.
//  * LDS across tokens: token t + 1 writes red_max in front of its first barrier and outp / red_sum behind it; every reader of token t's outp / red_*
//    (split_store_record included) has issued its reads before it arrives at that barrier, so one outp area serves all tokens.
struct PassSplitArgs {
    float* records;              // [ntok][n_heads][nsp][head_size + ATT_REC_PAD]
    const q4_half* q;            // [ntok][dim]
    const q4_half* key_cache;    // already offset to the layer
    const q4_half* value_cache;
    const int* pos;              // [ntok], ascending
    int ntok, dim, kv_dim, kv_mul, nsp;   // kv_mul query heads read the rows of K / V head h / kv_mul (rows kv_dim wide)
    size_t tok_stride;           // floats between two tokens' record areas
    float alpha;
};
// ROWS, the row form for a batch pass (q4_batch.h): one block per (head, chunk, listed row) runs this body for ONE token -- row t = list.row[z] with its
// own q, position, record area and cache (row_kv[t] / row_kv[PROMPT_PASS_MAX + t] plus the layer's offset) -- so a row's records are the ones a one-token pass of
// that sequence writes. a.key_cache / a.value_cache are then not read; a.nsp: the chunks this launch lays the records out by, the most of its rows' counts.
// A template value: with SPLIT_PASS the three trailing arguments are not read and the kernel is the code it was.
// SPLIT_RUNS, the run form for a batch pass whose slots carry several rows (q4_batch_set_prefill): one block per (head, chunk, listed run). A run is
// runs.len[z] adjacent rows of ONE sequence at consecutive positions, the first of them row t = list.row[z] (the last argument, which the other two
// values do not read -- it trails so that theirs sit where they sat): the block takes that row's q, position and
// record area as token 0's and the sequence's cache, and runs the token loop below over the run -- the chunk's K / V rows requested once for all of its
// rows, size_last from the run's last row, token i's records into row t + i's own area, a masked lane's V row the token's own (vown). This is the body the
// prompt pass holds to the step's bytes; a run of one row is the row form's block.
enum { SPLIT_PASS = 0, SPLIT_ROWS = 1, SPLIT_RUNS = 2 };
template <int U, int ROWS = SPLIT_PASS>
__global__ void __launch_bounds__(LA_WAVES * 64) prompt_split_attention_kernel(const PassSplitArgs a0, const PassRowList list, q4_half* const* row_kv, const long long loff,
                                                                               const PassRunList runs) {
    PassSplitArgs a = a0;
    if constexpr (ROWS != SPLIT_PASS) {
        const int t = list.row[blockIdx.z];
        a.records = a0.records + (size_t)t * a0.tok_stride;
        a.q = a0.q + (size_t)t * a0.dim;
        a.key_cache = row_kv[t] + loff;
        a.value_cache = row_kv[PROMPT_PASS_MAX + t] + loff;
        a.pos = a0.pos + t;
        a.ntok = ROWS == SPLIT_RUNS ? runs.len[blockIdx.z] : 1;
    }
    constexpr int LPR = 16, NW = LA_WAVES, R = 64 / LPR, stride = NW * R, CHUNK = stride * U, HS = LPR * 8;
    __shared__ __attribute__((aligned(16))) float lds[32 + NW * HS];
    float* red_max = lds;
    float* red_sum = lds + 16;
    float* outp = lds + 32;                                  // [NW][HS]
    const unsigned tid = threadIdx.x, lane = tid & 63u;
    const int wave = tid >> 6;
    const int row = lane / LPR, sub = lane % LPR;
    const int h = blockIdx.x, sp = blockIdx.y;
    const int ntok = a.ntok, kv_dim = a.kv_dim;
    const int rec = HS + ATT_REC_PAD;
    const int t_base = sp * CHUNK;
    const int size_last = __builtin_amdgcn_readfirstlane(a.pos[ntok - 1]) + 1;      // rows the pass may read: [0, size_last)
    if (NW < 16 && tid >= NW && tid < 16) { red_max[tid] = -INFINITY; red_sum[tid] = 0.f; }   // the reductions read 16 entries
    auto neutral = [&](int t) {      // a chunk wholly above pos[t]: attention_split_body's plain neutral words (m = -inf, l = 0)
        const f32x4 r4 = {-INFINITY, 0.f, 0.f, 0.f};
        *reinterpret_cast<f32x4*>(a.records + (size_t)t * a.tok_stride + ((size_t)h * a.nsp + sp) * rec + HS) = r4;
    };
    if (t_base >= size_last) {
        if ((int)tid < ntok) neutral((int)tid);
        return;
    }
    const q4_half* kh = a.key_cache + (size_t)(h / a.kv_mul) * HS + sub * 8;
    const q4_half* vh = a.value_cache + (size_t)(h / a.kv_mul) * HS + sub * 8;
    u32x4 kv[U], vv[U];
#pragma unroll
    for (int u = 0; u < U; u++) {
        const int r = t_base + wave * R + row + u * stride;
        const int rc = r < size_last ? r : size_last - 1;
        kv[u] = ld_nt(reinterpret_cast<const u32x4*>(kh + (size_t)rc * kv_dim));
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int u = 0; u < U; u++) {
        const int r = t_base + wave * R + row + u * stride;
        const int rc = r < size_last ? r : size_last - 1;
        vv[u] = ld_nt(reinterpret_cast<const u32x4*>(vh + (size_t)rc * kv_dim));
    }
    __builtin_amdgcn_sched_barrier(0);
    SplitArgs sa = {};
    sa.head_size = HS;
    for (int t = 0; t < ntok; t++) {
        const int size = __builtin_amdgcn_readfirstlane(a.pos[t]) + 1;
        if (t_base >= size) {                                // (block-uniform: no barrier is skipped by part of the block)
            if (tid == 0) neutral(t);
            continue;
        }
        const u32x4 qv = *reinterpret_cast<const u32x4*>(a.q + (size_t)t * a.dim + (size_t)h * HS + sub * 8);
        const u32x4 vown = *reinterpret_cast<const u32x4*>(vh + (size_t)(size - 1) * kv_dim);      // what split_live's clamp gives a masked lane
        float sc[U];
        float wmax = -INFINITY;
#pragma unroll
        for (int u = 0; u < U; u++) {
            const int r = t_base + wave * R + row + u * stride;
            float s = 0.f;
#pragma unroll
            for (int e = 0; e < 4; e++) s = __builtin_amdgcn_fdot2(as_h2(kv[u][e]), as_h2(qv[e]), s, false);
            s = row_sum<LPR>(s);
            s = round_h(s * a.alpha);
            sc[u] = r < size ? s : -INFINITY;
            wmax = fmaxf(wmax, sc[u]);
        }
        wmax = wave_max(wmax);
        if (lane == 0) red_max[wave] = wmax;
        __syncthreads();
        const float m = row16_max(red_max[lane & 15]);
        float acc[8];
#pragma unroll
        for (int e = 0; e < 8; e++) acc[e] = 0.f;
        float lsum = 0.f;
#pragma unroll
        for (int u = 0; u < U; u++) {
            const int r = t_base + wave * R + row + u * stride;
            const float p = expf(sc[u] - m);                 // 0 for masked positions (sc = -inf)
            if (sub == 0) lsum += p;
            const u32x4 vsel = r < size ? vv[u] : vown;
#pragma unroll
            for (int e = 0; e < 4; e++) {
                const h2 v2 = as_h2(vsel[e]);
                acc[2 * e] = __builtin_fmaf((float)v2.x, p, acc[2 * e]);
                acc[2 * e + 1] = __builtin_fmaf((float)v2.y, p, acc[2 * e + 1]);
            }
        }
        lsum = wave_sum(lsum);
        if (lane == 0) red_sum[wave] = lsum;
#pragma unroll
        for (int e = 0; e < 8; e++) {
            float v = acc[e];
            v += __shfl_xor(v, 32);
            v += __shfl_xor(v, 16);
            acc[e] = v;
        }
        if (lane < LPR) {
#pragma unroll
            for (int e = 0; e < 8; e++) outp[wave * HS + sub * 8 + e] = acc[e];
        }
        __syncthreads();
        const float l = row16_sum(red_sum[lane & 15]);
        sa.partials = a.records + (size_t)t * a.tok_stride;
        split_store_record<false, NW>(sa, Handoff{}, outp, m, l, h, sp, a.nsp);
    }
}

// The merge of a split pass: one block per (head, token) runs the step's merge arithmetic (combine_partials, chunk order) over the token's records and
// writes xb[t]. nsp_of_bin: the chunk count of the step's launch for the bin (graph bins), or 0: ceil((pos[t] + 1) / chunk), the count of a step that
// is handed its own size as the bin (no graphs) -- the chunks between the two are neutral either way.
__global__ void __launch_bounds__(128) prompt_merge_kernel(q4_half* xb, const float* records, const int* pos, int dim, int head_size, int nsp, size_t tok_stride,
                                                           int nsp_of_bin, int chunk) {
    const int h = blockIdx.x, t = blockIdx.y;
    const int n_merge = nsp_of_bin ? nsp_of_bin : (pos[t] + chunk) / chunk;
    const float* base = records + (size_t)t * tok_stride + (size_t)h * nsp * (head_size + ATT_REC_PAD);
    for (int n = threadIdx.x; n < head_size; n += blockDim.x)
        combine_partials<false>(xb + (size_t)t * dim + (size_t)h * head_size, base, head_size, n_merge, n);
}

// ... of the listed rows of a batch pass: row t = list.row[y] merges list.nsp_of_bin[y] chunks (0: those up to its own position), the step's count at its position
__global__ void __launch_bounds__(128) prompt_merge_rows_kernel(q4_half* xb, const float* records, const int* pos, int dim, int head_size, int nsp, size_t tok_stride,
                                                                const PassRowList list, int chunk) {
    const int h = blockIdx.x, t = list.row[blockIdx.y];
    const int n_merge = list.nsp_of_bin[blockIdx.y] ? list.nsp_of_bin[blockIdx.y] : (pos[t] + chunk) / chunk;
    const float* base = records + (size_t)t * tok_stride + (size_t)h * nsp * (head_size + ATT_REC_PAD);
    for (int n = threadIdx.x; n < head_size; n += blockDim.x)
        combine_partials<false>(xb + (size_t)t * dim + (size_t)h * head_size, base, head_size, n_merge, n);
}

// the n tokens' embedding rows, and the positions of the pass for its attention blocks
__global__ void prompt_embed_kernel(q4_half* xs, const q4_half* table, int dim, const int* tokens, const int* pPos, int* pos_arr) {
    const int u = blockIdx.x * blockDim.x + threadIdx.x, t = blockIdx.y;
    const int pos = *pPos + t;
    if (u == 0) pos_arr[t] = pos;
    if (u >= (dim >> 3)) return;
    const int token = tokens[pos];
    reinterpret_cast<u32x4*>(xs + (size_t)t * dim)[u] = reinterpret_cast<const u32x4*>(table + (size_t)token * dim)[u];
}

// what n per-token prompt steps leave: the last token's residual stream in RunState::x, both position words advanced by n (argmax_kernel's order)
__global__ void __launch_bounds__(1024) prompt_finish_kernel(q4_half* x, const q4_half* x_last, int dim, volatile int* pPos, int* pPosGpu, int n) {
    for (int u = threadIdx.x; u < (dim >> 3); u += blockDim.x) reinterpret_cast<u32x4*>(x)[u] = reinterpret_cast<const u32x4*>(x_last)[u];
    if (threadIdx.x == 0) {
        const int pos = *pPosGpu + n;
        __threadfence_system();
        *pPos = pos;
        *pPosGpu = pos;
    }
}

// ---- host ------------------------------------------------------------------------------------------
void pass_scratch_release(PassScratch* b) {
    for (void* d : {b->slab, (void*)b->records, (void*)b->logit_rows, (void*)b->lp_side, (void*)b->view, (void*)b->kv_stage})
        if (d) (void)hipFree(d);
    *b = PassScratch{};
}
void pass_release(Model* m) { pass_scratch_release(&m->pass); }

int prompt_pass_rows(Model* m, const Config* p) { return pass_scratch_rows(&m->pass, p); }
int pass_scratch_rows(PassScratch* scratch, const Config* p) {
    PassScratch& b = *scratch;
    if (!b.slab) {
        const size_t T = PROMPT_PASS_MAX, dim = p->dim, hidden = p->hidden_dim;
        const size_t sink_words = line_area_words(dim / 2);      // 32-bit words of one token's granule area
        const size_t vec = T * dim * sizeof(q4_half), hb = T * hidden * sizeof(q4_half);
        const size_t bytes = 3 * vec + hb + 256 + T * sink_words * 4;
        void* slab = nullptr;
        if (hipMalloc(&slab, bytes) != hipSuccess) { (void)hipGetLastError(); return Q4_ERR_ALLOC; }
        Q4_HIP(hipMemsetAsync(slab, 0, bytes, g_stream));
        char* c = (char*)slab;
        b.x = (q4_half*)c; c += vec;
        b.q = (q4_half*)c; c += vec;
        b.xb = (q4_half*)c; c += vec;
        b.hb = (q4_half*)c; c += hb;
        b.pos = (int*)c; c += 256;
        b.sink = (unsigned*)c;
        b.sink_stride = sink_words / 2;
        b.slab = slab;
    }
    return Q4_OK;
}

// The logits of a pass that runs the classifier (a verify pass; a prompt pass with records): [PROMPT_PASS_MAX][vocab] halves and, behind them, the
// PROMPT_PASS_MAX tokens the row form of the sampler leaves for the accept launch. pass_side_rows: the raw rows a pass under the sampler keeps for the
// records' look-up behind it (q4_logprobs.hip). Both allocated on first use, outside the launch path of later passes.
int pass_logit_rows(Model* m, const Config* p) {
    if (!m->pass.logit_rows && hipMalloc((void**)&m->pass.logit_rows, (size_t)PROMPT_PASS_MAX * p->vocab_size * sizeof(q4_half) + PROMPT_PASS_MAX * sizeof(int)) != hipSuccess) {
        (void)hipGetLastError(); m->pass.logit_rows = nullptr; return Q4_ERR_ALLOC;
    }
    return Q4_OK;
}
int pass_side_rows(Model* m, const Config* p) {
    if (!m->pass.lp_side && hipMalloc((void**)&m->pass.lp_side, (size_t)PROMPT_PASS_MAX * p->vocab_size * sizeof(q4_half)) != hipSuccess) {
        (void)hipGetLastError(); m->pass.lp_side = nullptr; return Q4_ERR_ALLOC;
    }
    return Q4_OK;
}

// The draft view of a verify pass with logit stages (spec_verify.h): seq_len tokens by absolute position, allocated on first use
int pass_draft_view(Model* m, const Config* p) {
    if (!m->pass.view && hipMalloc((void**)&m->pass.view, (size_t)p->seq_len * sizeof(int)) != hipSuccess) {
        (void)hipGetLastError(); m->pass.view = nullptr; return Q4_ERR_ALLOC;
    }
    return Q4_OK;
}

// The staging rows of a pass over the FP8 cache (prompt_pass_kv8.h): [2][PROMPT_PASS_MAX][kv_dim] halves, the tokens' K rows and behind them their V
// rows between the q/k/v launch and the append launch, allocated on first use
static int pass_kv_stage_rows(Model* m, int kv_dim) {
    if (!m->pass.kv_stage && hipMalloc((void**)&m->pass.kv_stage, (size_t)2 * PROMPT_PASS_MAX * kv_dim * sizeof(q4_half)) != hipSuccess) {
        (void)hipGetLastError(); m->pass.kv_stage = nullptr; return Q4_ERR_ALLOC;
    }
    return Q4_OK;
}

// The split passes' flash-decode records: the pass's own buffer (never RunState::att, whose words are validated by tag), allocated on the first split
// pass of the model for the longest context it can meet -- PROMPT_PASS_MAX tokens x heads x chunks x (head_size + ATT_REC_PAD) floats.
int pass_records_of(PassScratch* b, size_t floats) {
    if (b->record_floats >= floats) return Q4_OK;
    if (b->records) {
        Q4_HIP(hipStreamSynchronize(g_stream));              // a pass that reads the old area may still be in flight
        (void)hipFree(b->records);
        b->records = nullptr;
        b->record_floats = 0;
    }
    if (hipMalloc((void**)&b->records, floats * sizeof(float)) != hipSuccess) { (void)hipGetLastError(); b->records = nullptr; return Q4_ERR_ALLOC; }
    b->record_floats = floats;
    return Q4_OK;
}

static void fill_mat(GemvMat& m, const QWeight* w) { m.w = w->weight; m.z = w->zeros; m.s = w->scales; }
static void fill_geom(GemvArgs& a, int K, int N) {
    const QGeom g = make_geom(K, N);
    a.K = K; a.N = N; a.pw4 = g.pw4; a.pzh = g.pzh; a.sh = g.sh; a.nslots = g.nslots;
    a.loff = -1;
}

// The down projection of a hidden size the FFN pair launch does not take, as the step runs it (launch_gemv_plain): the two-part K split whose parts fill
// three whole k-slots and a last one of at most 32 units -- the shared half slot, gemv_q4_kernel<MODE_PLAIN, 4, 4, false, 0, 2, true> or its strips
// form -- which the step takes only with the K split and the half slot on (q4_set_ksplit 0 / 4 and q4_set_half_tail(0) select other arithmetic: no pass).
// Hidden 14336: 448 units, ku = 224 = 3 x 64 + 32.
static bool pass_down_half_covers(int dim, int hidden) {
    if ((hidden & 31) || ffn_pair_covers(dim, hidden)) return false;
    if (!g_ksplit || g_ksplit == 4 || !g_half_tail || g_ablate != 0) return false;
    const QGeom g = make_geom(hidden, dim);
    const int ku = (divUp(g.pw4, 2) + 3) & ~3;
    return g.nslots >= 5 && g.nslots <= 8 && divUp(ku, 64) == 4 && ku - 192 <= 32 && ku * 2 >= g.pw4;
}
// Llama-2-13B's shape (q4_set_pass_13b): dim 5120 as forty 128-wide heads, multi-head, hidden 13824, an fp16 cache -- and the step on the forms the pass
// restates: the K = 5120 matrices in strip_k5120's geometry (160 units, 40 scales and 5 zero words per column: two whole k-slots and the shared half
// slot), the product's GEMV forms (every K = 5120 form of GEMV_PRODUCT puts an even column's half-slot terms in lanes 0 - 31; the profiling library's
// other forms are not restated here: no pass), the half slot and the K split in force (pass_down_half_covers: q4_set_half_tail(0) moves q/k/v, o-proj,
// gate/up AND down to other arithmetic, q4_set_ksplit(0 | 4) the down projection). Grouped-query, the FP8 cache (also with q4_set_pass_kv8 on) and other
// hidden sizes at this width keep their steps: admit what is tested.
static bool pass_13b_covers(const Config* p, const Model* m) {
    const int dim = p->dim, hidden = p->hidden_dim;
    if (!m->pass_13b || m->kv_format != Q4_KV_FP16 || dim != 5120 || p->n_heads * 128 != dim || p->n_heads != p->n_kv_heads || hidden != 13824) return false;
    if (g_gemv_form != GEMV_PRODUCT || !pass_down_half_covers(dim, hidden)) return false;
    for (const int n : {dim, hidden}) {
        const QGeom g = make_geom(dim, n);
        if (g.pw4 != 160 || g.sh != 40 || g.pzh != 5 || g.nslots != 3) return false;
    }
    return (3 * dim / 4) % PP13_QKV_WAVES == 0 && (dim / 2) % PP13_O_WAVES == 0 && (hidden / 2) % PP13_FFN_WAVES == 0 && dim % PP_WAVES == 0 &&
           stream_cu_count() == cu_count();
}
#ifndef Q4_PP13_MIN                    // (make exp EXPFLAGS=-DQ4_PP13_MIN=2: passes of two and three positions at dim 5120 too, for tools/bench_pass_13b.py's section b)
#define Q4_PP13_MIN 4
#endif
int prompt_pass_min(const Config* p) { return p->dim == 5120 ? Q4_PP13_MIN : 2; }
// The two 4096-wide layer shapes the pass kernels restate, in ONE place for the passes' admission and the batch's (batch_pass_covers): 128-wide heads;
// multi-head with a hidden size the FFN pair launch takes (the down projection as the two-part K split in three k-slots, no shared half slot: Llama-2-7B),
// or -- gqa: the caller admits grouped-query models -- four query heads per K / V head and the half-slot down form (Mistral-7B, Llama-3-8B: what the tests run)
static bool pass_shape_4096_covers(const Config* p, bool gqa) {
    const int dim = p->dim, hidden = p->hidden_dim;
    if (dim != 4096 || p->n_heads * 128 != dim || (hidden & 31)) return false;
    if (p->n_heads != p->n_kv_heads) {
        if (!gqa || p->n_kv_heads < 1 || p->n_heads != 4 * p->n_kv_heads) return false;
        return pass_down_half_covers(dim, hidden) && stream_cu_count() == cu_count();
    }
    if (!ffn_pair_covers(dim, hidden)) return false;
    const QGeom g = make_geom(hidden, dim);
    const int ku = (divUp(g.pw4, 2) + 3) & ~3;
    if (divUp(ku, 64) != 3 || ku - 128 <= 32 || ku * 2 < g.pw4) return false;        // the two-part K split in three k-slots, no shared half slot
    return stream_cu_count() == cu_count();
}
bool prompt_pass_covers(const Config* p, const Model* m) {
    if (!p || !m || !m->rope_table || !m->sync) return false;
    if (p->dim == 5120) return pass_13b_covers(p, m);
    if (m->kv_format != Q4_KV_FP16) {       // the FP8 cache: q4_set_pass_kv8, and a head the append and attention launches of prompt_pass_kv8.hip take (128, checked below)
        if (m->kv_format != Q4_KV_FP8 || !m->pass_kv8 || !m->k_exp || !m->v_exp || !kv8_head_size_ok(p->n_heads > 0 ? p->dim / p->n_heads : 0)) return false;
    }
    return pass_shape_4096_covers(p, m->pass_gqa);      // (grouped-query: q4_set_pass_gqa)
}

constexpr int TB = PP_WAVES * 64;
constexpr size_t SMEM_NORM = prompt_gemv_lds<2, 1, true, 4>(), SMEM_O = prompt_gemv_lds<2, 1, false, 4>(), SMEM_DOWN = prompt_gemv_lds<3, 2, false, 2>();
constexpr size_t SMEM_DOWN_HALF = prompt_gemv_lds<4, 2, false, PP_DOWN_HALF_G>();
static_assert(SMEM_NORM <= 64 * 1024 && SMEM_DOWN <= 64 * 1024 && (SMEM_DOWN_HALF <= 64 * 1024 || PP_DOWN_HALF_G > 1), "no LDS opt-in in the shipped form");
constexpr size_t SMEM_NORM13 = prompt_gemv_lds<3, 1, true, PP13_G>(), SMEM_QKV13 = prompt_gemv_lds<3, 1, true, PP13_QKV_G>(), SMEM_O13 = prompt_gemv_lds<3, 1, false, 4>();
static_assert(SMEM_NORM13 <= 64 * 1024 && SMEM_O13 <= 64 * 1024, "no LDS opt-in in the shipped form");

// The three launches of a layer behind attention -- o-proj + residual, rmsnorm + gate/up + SiLU, down projection + residual -- over rows 0 .. n - 1 of a
// scratch. A row's values depend on that row alone, so the prompt and verify passes and the batch pass (q4_batch.h: rows of different sequences) share them.
static int pass_layer_tail(const Config* p, const PerLayerWeight* L, const PassScratch* b, int n) {
    const int dim = p->dim, hidden = p->hidden_dim;
    const bool down_half = !ffn_pair_covers(dim, hidden);    // (prompt_pass_covers: then the shared-half-slot form)
    const bool k13 = dim == 5120;                            // (prompt_pass_covers: q4_set_pass_13b's shape, K = 5120 in two k-slots and the shared half slot)
    if (SMEM_DOWN_HALF > 64 * 1024)     // (an experiment build only)
        Q4_TRY(lds_opt_in((const void*)prompt_gemv_kernel<MODE_PLAIN, 4, 2, false, 2, PP_DOWN_HALF_G, PP_WAVES, false, true>, SMEM_DOWN_HALF));
    {   // o-proj + residual (K = 5120: a column pair per wave, the shared half slot)
        GemvArgs a = {};
        fill_geom(a, dim, dim);
        fill_mat(a.m[0], &L->wq_o);
        a.out[0] = b->x; a.x = b->xb; a.accum = 1;
        if (k13) Q4_LAUNCH((prompt_gemv_kernel<MODE_PLAIN, 3, 2, false, 1, 4, PP13_O_WAVES, false, true>), dim3(dim / (PP13_O_WAVES * 2)), dim3(PP13_O_WAVES * 64), SMEM_O13, a, n);
        else Q4_LAUNCH((prompt_gemv_kernel<MODE_PLAIN, 2, 1, false, 1, 4, PP_WAVES>), dim3(dim / PP_WAVES), dim3(TB), SMEM_O, a, n);
        Q4_LAUNCH_CHECK();
    }
    {   // rmsnorm + gate/up + SiLU (K = 5120: a column pair of gate and of up per wave, the strips' pair units)
        GemvArgs a = {};
        fill_geom(a, dim, hidden);
        fill_mat(a.m[0], &L->wq_gate); fill_mat(a.m[1], &L->wq_up);
        a.out[0] = b->hb; a.x = b->x; a.rms_w = L->rms_ffn_weight;
        if (k13) Q4_LAUNCH((prompt_gemv_kernel<MODE_FFN, 3, 2, true, 1, PP13_G, PP13_FFN_WAVES, false, true>), dim3(hidden / (PP13_FFN_WAVES * 2)), dim3(PP13_FFN_WAVES * 64), SMEM_NORM13, a, n);
        else Q4_LAUNCH((prompt_gemv_kernel<MODE_FFN, 2, 3, true, 1, 4, PP_WAVES>), dim3(divUp(hidden, PP_WAVES * 3)), dim3(TB), SMEM_NORM, a, n);
        Q4_LAUNCH_CHECK();
    }
    if (down_half) {   // down projection + residual, the shared-half-slot form: two k-parts of three slots and a shared one, a column pair per wave
        GemvArgs a = {};
        fill_geom(a, hidden, dim);
        fill_mat(a.m[0], &L->wq_down);
        a.ku = (divUp(a.pw4, 2) + 3) & ~3;
        a.out[0] = b->x; a.x = b->hb; a.accum = 1;
        Q4_LAUNCH((prompt_gemv_kernel<MODE_PLAIN, 4, 2, false, 2, PP_DOWN_HALF_G, PP_WAVES, false, true>), dim3(dim / (PP_WAVES / 2 * 2)), dim3(TB), SMEM_DOWN_HALF, a, n);
        Q4_LAUNCH_CHECK();
    } else {   // down projection + residual: two k-parts, part 0 then part 1
        GemvArgs a = {};
        fill_geom(a, hidden, dim);
        fill_mat(a.m[0], &L->wq_down);
        a.ku = (divUp(a.pw4, 2) + 3) & ~3;
        a.out[0] = b->x; a.x = b->hb; a.accum = 1;
        Q4_LAUNCH((prompt_gemv_kernel<MODE_PLAIN, 3, 2, false, 2, 2, PP_WAVES>), dim3(dim / (PP_WAVES / 2 * 2)), dim3(TB), SMEM_DOWN, a, n);
        Q4_LAUNCH_CHECK();
    }
    return Q4_OK;
}

// The layer loop of a pass, shared by the prompt pass below and the verify pass (spec_verify.hip): rows 0 .. n - 1 of the model's scratch rows hold the
// positions' residual streams going in (and pos[t] their positions), and their final residual streams coming out. pos0: the position of row 0 as the
// host knows it (the device position when the pass runs) -- which attention launch the layers take is decided from it (pass_attention_plan), the kernels
// read the positions from pos[].
int prompt_pass_layers(const Config* p, RunState* s, const TransformerWeights* w, Model* m, int pos0, int n) {
    if (!prompt_pass_covers(p, m) || n < 2 || n > PROMPT_PASS_MAX) return Q4_ERR_ARG;
    const int dim = p->dim, head_size = dim / p->n_heads;
    const int kv_mul = p->n_heads / p->n_kv_heads, kv_dim = dim / kv_mul;
    const bool k13 = dim == 5120;                            // (prompt_pass_covers: q4_set_pass_13b's shape, K = 5120 in two k-slots and the shared half slot)
    Q4_TRY(prompt_pass_rows(m, p));
    PassScratch* const b = &m->pass;
    PassAttention plan = {};
    if (!pass_attention_plan(p, s, pos0, n, &plan)) return Q4_ERR_ARG;
    const bool split = att_is_split(plan.form);
    // The FP8 cache (q4_set_pass_kv8; prompt_pass_kv8.h): q/k/v into the staging rows, the append launch, attention over the byte caches
    const bool kv8 = m->kv_format == Q4_KV_FP8;
    q4_half* k_stage = nullptr;
    q4_half* v_stage = nullptr;
    if (kv8) {
        if (head_size != 128 || pos0 < 0 || pos0 + n > p->seq_len || (!split && pos0 + n > PASS_CONTEXT_MIN)) return Q4_ERR_ARG;   // (the one-pass row form keeps 256 scores)
        Q4_TRY(pass_kv_stage_rows(m, kv_dim));
        k_stage = m->pass.kv_stage;
        v_stage = k_stage + (size_t)PROMPT_PASS_MAX * kv_dim;
    }
    const int rec = head_size + ATT_REC_PAD;
    const size_t tok_stride = (size_t)p->n_heads * plan.nsp * rec;
    if (split) {
        if (head_size != 128 || pos0 + n > p->seq_len) return Q4_ERR_ARG;
        const int most = divUp(p->seq_len, 64) > plan.nsp ? divUp(p->seq_len, 64) : plan.nsp;      // the smallest chunk's count over the whole context
        Q4_TRY(pass_records_of(b, (size_t)PROMPT_PASS_MAX * p->n_heads * most * rec));
    }
    const float alpha = (float)(1.0 / sqrt((double)head_size));                     // llama2_q4.cu:273
    const unsigned natt = (unsigned)p->n_heads * 4u;
    for (int l = 0; l < p->n_layers; l++) {
        const PerLayerWeight* L = &w->layers[l];
        const long long loff = (long long)l * p->seq_len * kv_dim;
        if (k13) {   // rmsnorm + q/k/v + RoPE + K/V rows at K = 5120: 3 x 1280 column groups, the step's pairs (i, i + 1 of a head) on the half slot
            GemvArgs a = {};
            fill_geom(a, dim, dim);
            fill_mat(a.m[0], &L->wq_q); fill_mat(a.m[1], &L->wq_k); fill_mat(a.m[2], &L->wq_v);
            a.out[0] = b->q; a.out[1] = s->key_cache; a.out[2] = s->value_cache;
            a.x = b->x; a.rms_w = L->rms_att_weight; a.pPos = s->pos; a.loff = loff;
            a.rope = 1; a.head_size = head_size; a.rope_theta = p->rope_theta; a.rope_table = m->rope_table;
            Q4_LAUNCH((prompt_gemv_kernel<MODE_QKV, 3, 4, true, 1, PP13_QKV_G, PP13_QKV_WAVES, false, true>), dim3(3 * dim / (PP13_QKV_WAVES * 4)), dim3(PP13_QKV_WAVES * 64), SMEM_QKV13, a, n);
            Q4_LAUNCH_CHECK();
        } else if (kv_mul > 1) {   // ... grouped-query: 1024 column groups of q, then 256 of k and of v, in six-wave blocks
            GemvArgs a = {};
            fill_geom(a, dim, dim);
            a.N_kv = kv_dim;
            fill_mat(a.m[0], &L->wq_q); fill_mat(a.m[1], &L->wq_k); fill_mat(a.m[2], &L->wq_v);
            a.out[0] = b->q; a.out[1] = kv8 ? k_stage : s->key_cache; a.out[2] = kv8 ? v_stage : s->value_cache;
            a.x = b->x; a.rms_w = L->rms_att_weight; a.pPos = s->pos; a.loff = loff; a.kv_stage = kv8 ? 1 : 0;
            a.rope = 1; a.head_size = head_size; a.rope_theta = p->rope_theta; a.rope_table = m->rope_table;
            const int groups = (dim + 2 * kv_dim) / 4;
            if (groups % PP_QKV_GQA_WAVES) return Q4_ERR_ARG;
            if (kv8) Q4_LAUNCH((prompt_gemv_kernel<MODE_QKV, 2, 4, true, 1, 4, PP_QKV_GQA_WAVES, true, false, true>), dim3(groups / PP_QKV_GQA_WAVES), dim3(PP_QKV_GQA_WAVES * 64), SMEM_NORM, a, n);
            else Q4_LAUNCH((prompt_gemv_kernel<MODE_QKV, 2, 4, true, 1, 4, PP_QKV_GQA_WAVES, true>), dim3(groups / PP_QKV_GQA_WAVES), dim3(PP_QKV_GQA_WAVES * 64), SMEM_NORM, a, n);
            Q4_LAUNCH_CHECK();
        } else {   // rmsnorm + q/k/v + RoPE + K/V rows
            GemvArgs a = {};
            fill_geom(a, dim, dim);
            fill_mat(a.m[0], &L->wq_q); fill_mat(a.m[1], &L->wq_k); fill_mat(a.m[2], &L->wq_v);
            a.out[0] = b->q; a.out[1] = kv8 ? k_stage : s->key_cache; a.out[2] = kv8 ? v_stage : s->value_cache;
            a.x = b->x; a.rms_w = L->rms_att_weight; a.pPos = s->pos; a.loff = loff; a.kv_stage = kv8 ? 1 : 0;
            a.rope = 1; a.head_size = head_size; a.rope_theta = p->rope_theta; a.rope_table = m->rope_table;
            if (kv8) Q4_LAUNCH((prompt_gemv_kernel<MODE_QKV, 2, 4, true, 1, 4, PP_QKV_WAVES, false, false, true>), dim3(3 * dim / (PP_QKV_WAVES * 4)), dim3(PP_QKV_WAVES * 64), SMEM_NORM, a, n);
            else Q4_LAUNCH((prompt_gemv_kernel<MODE_QKV, 2, 4, true, 1, 4, PP_QKV_WAVES>), dim3(3 * dim / (PP_QKV_WAVES * 4)), dim3(PP_QKV_WAVES * 64), SMEM_NORM, a, n);
            Q4_LAUNCH_CHECK();
        }
        if (kv8) {   // the FP8 cache: the tokens' rows appended (bytes and exponents, also those of a verify pass's drafts), then attention over rows [0, pos[t]] of the byte caches
            const size_t eoff = (size_t)l * p->n_kv_heads * p->seq_len;
            const PassKv8 c = {(uint8_t*)s->key_cache + loff, (uint8_t*)s->value_cache + loff, m->k_exp + eoff, m->v_exp + eoff, p->n_heads, head_size, kv_mul, kv_dim,
                               p->seq_len, b->pos, n};
            Q4_TRY(launch_pass_kv8_append(c, k_stage, v_stage));
            if (split) {
                Q4_TRY(launch_pass_kv8_split(c, b->records, tok_stride, b->q, dim, alpha, plan.chunk, plan.nsp));
                Q4_LAUNCH(prompt_merge_kernel, dim3((unsigned)p->n_heads, (unsigned)n), dim3(128), 0, b->xb, (const float*)b->records, (const int*)b->pos, dim, head_size,
                          plan.nsp, tok_stride, plan.nsp_of_bin, plan.chunk);
                Q4_LAUNCH_CHECK();
            } else {
                Q4_TRY(launch_pass_kv8_attention(c, b->xb, b->q, dim, alpha));
            }
        } else if (split) {   // attention in the split-context bins: one block per (head, chunk) loops over the tokens, then the step's merge per (head, token)
            const PassSplitArgs a = {b->records, b->q, s->key_cache + loff, s->value_cache + loff, b->pos, n, dim, kv_dim, kv_mul, plan.nsp, tok_stride, alpha};
            const dim3 grid((unsigned)p->n_heads, (unsigned)plan.nsp);
            const PassRowList none = {};
            if (plan.chunk == 64) Q4_LAUNCH(prompt_split_attention_kernel<2>, grid, dim3(LA_WAVES * 64), 0, a, none, (q4_half* const*)nullptr, 0ll, PassRunList{});
            else if (plan.chunk == 128) Q4_LAUNCH(prompt_split_attention_kernel<4>, grid, dim3(LA_WAVES * 64), 0, a, none, (q4_half* const*)nullptr, 0ll, PassRunList{});
            else Q4_LAUNCH(prompt_split_attention_kernel<8>, grid, dim3(LA_WAVES * 64), 0, a, none, (q4_half* const*)nullptr, 0ll, PassRunList{});
            Q4_LAUNCH_CHECK();
            Q4_LAUNCH(prompt_merge_kernel, dim3((unsigned)p->n_heads, (unsigned)n), dim3(128), 0, b->xb, (const float*)b->records, (const int*)b->pos, dim, head_size,
                      plan.nsp, tok_stride, plan.nsp_of_bin, plan.chunk);
            Q4_LAUNCH_CHECK();
        } else {   // attention below bin 512: the V-slice units
            const AttArgs a = {b->xb, b->q, s->key_cache + loff, s->value_cache + loff, head_size, kv_mul, kv_dim, b->pos, alpha, 256, nullptr};
            Q4_LAUNCH(prompt_attention_kernel, dim3((unsigned)n * natt), dim3(LA16_WAVES * 64), LA16_LDS, a, (const int*)b->pos, (u32x2v*)b->sink, (unsigned)b->sink_stride,
                      (unsigned)p->n_heads, natt, dim);
            Q4_LAUNCH_CHECK();
        }
        Q4_TRY(pass_layer_tail(p, L, b, n));
    }
    return Q4_OK;
}

// ---- the batch pass (q4_batch.h) ----------------------------------------------------------------------------------------------
// The shapes a batch pass takes: prompt_pass_covers' two 4096-wide shapes with the fp16 cache -- Llama-2-7B's, and the grouped-query one whatever
// q4_set_pass_gqa says (the switch guards the token loop's passes; a batch is asked for by name). Admit what is tested.
bool batch_pass_covers(const Config* p, const Model* m) {
    if (!p || !m || !m->rope_table || !m->sync || m->kv_format != Q4_KV_FP16 || p->n_heads < 1) return false;
    if (p->n_heads != p->n_kv_heads && (p->dim + 2 * (p->dim / 4)) / 4 % PP_QKV_GQA_WAVES) return false;      // (the grouped-query q/k/v grid: whole blocks)
    return pass_shape_4096_covers(p, true) && verify_cls_covers(p->dim, p->vocab_size);
}

// The layer loop over the n rows of a batch pass: rows 0 .. n - 1 of the batch's scratch hold the rows' residual streams going in and coming out,
// b->pos[t] (device) their positions, kv (device) their cache bases; pos_host[t]: the positions as the host knows them -- a slot advances by its row
// count per pass (q4_batch_plan_rows), so the host always does -- from which each row's attention form is planned as the step at that position would take it (pass_attention_plan with
// one position). Per layer: q/k/v in its ROWS form, at most one V-slice launch and one split + merge pair per chunk size present among the rows, then
// pass_layer_tail. Every launch names its rows by value; nothing waits in-launch.
// seq (q4_batch_set_prefill: a slot may carry several rows): seq[t] names row t's sequence, the rows of one sequence adjacent and at consecutive ascending
// positions; nullptr: every row another sequence. Adjacent rows of one sequence inside one chunk-size list form a run; a list with a run of two or more
// rows takes the split launch's run form (one block per (head, chunk, run): the chunk's K / V rows loaded once per run), any other list the row form.
#ifdef Q4_PROFILING            // the profiling build only: q4_set_batch_run_form(0) runs every list in the row form (tools/bench_batch_prefill.py)
static int g_batch_run_form = 1;
static bool batch_run_form() { return g_batch_run_form != 0; }
#else
static constexpr bool batch_run_form() { return true; }
#endif
int batch_pass_layers(const Config* p, const RunState* s, const TransformerWeights* w, Model* m, PassScratch* b, const int* pos_host, int n, q4_half* const* kv,
                      const int* seq) {
    if (!batch_pass_covers(p, m) || n < 1 || n > PROMPT_PASS_MAX || !b->slab || !kv) return Q4_ERR_ARG;
    const int dim = p->dim, head_size = dim / p->n_heads;
    const int kv_mul = p->n_heads / p->n_kv_heads, kv_dim = dim / kv_mul;
    PassRowList vslice = {};
    // list: the rows of this chunk size (the row form and the merge); heads / runs: the first row and the length of each run among them
    struct SplitRows { PassRowList list; int chunk, nsp; PassRowList heads; PassRunList runs; bool run_form; } split[3] = {};
    split[0].chunk = 64; split[1].chunk = 128; split[2].chunk = 256;
    for (int t = 0; t < n; t++) {
        PassAttention plan = {};
        if (pos_host[t] < 0 || pos_host[t] >= p->seq_len || !pass_attention_plan(p, s, pos_host[t], 1, &plan)) return Q4_ERR_ARG;
        if (seq && t > 0 && seq[t] == seq[t - 1] && pos_host[t] != pos_host[t - 1] + 1) return Q4_ERR_ARG;
        if (!att_is_split(plan.form)) { vslice.row[vslice.n++] = t; continue; }
        SplitRows* f = plan.chunk == 64 ? &split[0] : plan.chunk == 128 ? &split[1] : plan.chunk == 256 ? &split[2] : nullptr;
        if (!f || head_size != 128) return Q4_ERR_ARG;
        if (seq && f->list.n && f->list.row[f->list.n - 1] == t - 1 && seq[t] == seq[t - 1]) {
            f->runs.len[f->heads.n - 1]++;
            f->run_form = batch_run_form();
        } else {
            f->runs.len[f->heads.n] = 1;
            f->heads.row[f->heads.n++] = t;
        }
        f->list.nsp_of_bin[f->list.n] = plan.nsp_of_bin;
        f->list.row[f->list.n++] = t;
        if (plan.nsp > f->nsp) f->nsp = plan.nsp;
    }
    const int rec = head_size + ATT_REC_PAD;
    int most = divUp(p->seq_len, 64);
    for (const SplitRows& f : split) if (f.nsp > most) most = f.nsp;
    if (split[0].list.n || split[1].list.n || split[2].list.n) Q4_TRY(pass_records_of(b, (size_t)PROMPT_PASS_MAX * p->n_heads * most * rec));
    const float alpha = (float)(1.0 / sqrt((double)head_size));                     // llama2_q4.cu:273
    const unsigned natt = (unsigned)p->n_heads * 4u;
    for (int l = 0; l < p->n_layers; l++) {
        const PerLayerWeight* L = &w->layers[l];
        const long long loff = (long long)l * p->seq_len * kv_dim;
        {   // rmsnorm + q/k/v + RoPE, row t rotated by its own position, its K / V row into its own sequence's cache
            GemvArgs a = {};
            fill_geom(a, dim, dim);
            a.N_kv = kv_mul > 1 ? kv_dim : 0;
            fill_mat(a.m[0], &L->wq_q); fill_mat(a.m[1], &L->wq_k); fill_mat(a.m[2], &L->wq_v);
            a.out[0] = b->q; a.row_kv = kv;
            a.x = b->x; a.rms_w = L->rms_att_weight; a.pPos = b->pos; a.loff = loff;
            a.rope = 1; a.head_size = head_size; a.rope_theta = p->rope_theta; a.rope_table = m->rope_table;
            if (kv_mul > 1) Q4_LAUNCH((prompt_gemv_kernel<MODE_QKV, 2, 4, true, 1, 4, PP_QKV_GQA_WAVES, true, false, false, true>), dim3((dim + 2 * kv_dim) / 4 / PP_QKV_GQA_WAVES), dim3(PP_QKV_GQA_WAVES * 64), SMEM_NORM, a, n);
            else Q4_LAUNCH((prompt_gemv_kernel<MODE_QKV, 2, 4, true, 1, 4, PP_QKV_WAVES, false, false, false, true>), dim3(3 * dim / (PP_QKV_WAVES * 4)), dim3(PP_QKV_WAVES * 64), SMEM_NORM, a, n);
            Q4_LAUNCH_CHECK();
        }
        if (vslice.n) {   // the rows below bin 512: the V-slice units, each row over its own cache
            const AttArgs a = {b->xb, b->q, nullptr, nullptr, head_size, kv_mul, kv_dim, b->pos, alpha, 256, nullptr};
            Q4_LAUNCH(prompt_attention_rows_kernel, dim3((unsigned)vslice.n * natt), dim3(LA16_WAVES * 64), LA16_LDS, a, (const int*)b->pos, (u32x2v*)b->sink, (unsigned)b->sink_stride,
                      (unsigned)p->n_heads, natt, dim, vslice, kv, loff);
            Q4_LAUNCH_CHECK();
        }
        for (const SplitRows& f : split) {   // the rows in the split-context bins, by chunk size: one block per (head, chunk, row), then the step's merge per (head, row)
            if (!f.list.n) continue;
            const size_t tok_stride = (size_t)p->n_heads * f.nsp * rec;
            const PassSplitArgs a = {b->records, b->q, nullptr, nullptr, b->pos, 1, dim, kv_dim, kv_mul, f.nsp, tok_stride, alpha};
            if (f.run_form) {   // ... one block per (head, chunk, run) where a sequence has several rows here; the merge stays per row, each with its own chunk count
                const dim3 grid((unsigned)p->n_heads, (unsigned)f.nsp, (unsigned)f.heads.n);
                if (f.chunk == 64) Q4_LAUNCH((prompt_split_attention_kernel<2, SPLIT_RUNS>), grid, dim3(LA_WAVES * 64), 0, a, f.heads, kv, loff, f.runs);
                else if (f.chunk == 128) Q4_LAUNCH((prompt_split_attention_kernel<4, SPLIT_RUNS>), grid, dim3(LA_WAVES * 64), 0, a, f.heads, kv, loff, f.runs);
                else Q4_LAUNCH((prompt_split_attention_kernel<8, SPLIT_RUNS>), grid, dim3(LA_WAVES * 64), 0, a, f.heads, kv, loff, f.runs);
            } else {
                const dim3 grid((unsigned)p->n_heads, (unsigned)f.nsp, (unsigned)f.list.n);
                if (f.chunk == 64) Q4_LAUNCH((prompt_split_attention_kernel<2, SPLIT_ROWS>), grid, dim3(LA_WAVES * 64), 0, a, f.list, kv, loff, PassRunList{});
                else if (f.chunk == 128) Q4_LAUNCH((prompt_split_attention_kernel<4, SPLIT_ROWS>), grid, dim3(LA_WAVES * 64), 0, a, f.list, kv, loff, PassRunList{});
                else Q4_LAUNCH((prompt_split_attention_kernel<8, SPLIT_ROWS>), grid, dim3(LA_WAVES * 64), 0, a, f.list, kv, loff, PassRunList{});
            }
            Q4_LAUNCH_CHECK();
            Q4_LAUNCH(prompt_merge_rows_kernel, dim3((unsigned)p->n_heads, (unsigned)f.list.n), dim3(128), 0, b->xb, (const float*)b->records, (const int*)b->pos, dim, head_size,
                      f.nsp, tok_stride, f.list, f.chunk);
            Q4_LAUNCH_CHECK();
        }
        Q4_TRY(pass_layer_tail(p, L, b, n));
    }
    return Q4_OK;
}

int run_prompt_pass(const Config* p, RunState* s, const TransformerWeights* w, Model* m, int pos0, int n, const Sampler* sampler) {
    if (!prompt_pass_covers(p, m) || n < 2 || n > PROMPT_PASS_MAX) return Q4_ERR_ARG;
    const int dim = p->dim;
    const bool records = m->logprobs_k >= 0;               // (admitted with records on: q4_set_pass_logprobs, q4_passes.hip)
    if (records && (!m->pass_logprobs || !verify_cls_covers(dim, p->vocab_size))) return Q4_ERR_ARG;
    Q4_TRY(prompt_pass_rows(m, p));
    if (records) Q4_TRY(pass_logit_rows(m, p));
    const PassScratch* const b = &m->pass;
    // q4_set_pass_stages: state by position -- the guide's automaton, Mirostat's mu -- is put to NONE at the pass's positions, in stream order in front of
    // the pass, as run_transformer_steps_screenable does for a prompt group (prompt_pass_tokens admits either only with the switch on)
    Q4_TRY(stages_clear_positions(sampler, m, pos0, n));
    Q4_LAUNCH(prompt_embed_kernel, dim3(divUp(dim >> 3, 256), n), dim3(256), 0, b->x, w->token_embedding_table, dim, (const int*)s->shared_data->tokens,
              (const int*)s->pos, b->pos);
    Q4_LAUNCH_CHECK();
    Q4_TRY(prompt_pass_layers(p, s, w, m, pos0, n));
    if (records) {      // what n prompt steps with records leave besides: records pos0 .. pos0 + n - 1 (the target of row r is the ring's next token) and, in
        // RunState::logits, the last position's logits. The classifier of the verify pass over the n rows, then the row form of the record launch
        Q4_TRY(launch_verify_cls(b->logit_rows, b->x, w->rms_final_weight, w->wcls, dim, p->vocab_size, n));
        Q4_TRY(launch_logprobs_rows(m, p, s, b->logit_rows, p->vocab_size, n, LP_TARGET));
        Q4_HIP(hipMemcpyAsync(s->logits, b->logit_rows + (size_t)(n - 1) * p->vocab_size, (size_t)p->vocab_size * sizeof(q4_half), hipMemcpyDeviceToDevice, g_stream));
    }
    Q4_LAUNCH(prompt_finish_kernel, dim3(1), dim3(1024), 0, s->x, (const q4_half*)(b->x + (size_t)(n - 1) * dim), dim, &(s->shared_data->pos), s->pos, n);
    Q4_LAUNCH_CHECK();
    return Q4_OK;
}

}  // namespace q4

#ifdef Q4_PROFILING
// a measurement knob of the profiling build (q4_kernels.hip lists the others): 0 runs every split-context list of a batch pass in the row form
extern "C" void q4_set_batch_run_form(int on) { q4::g_batch_run_form = on; }
#endif
