// cls_screen.h -- the classifier of a GREEDY step without streaming every fp16 row: the token loop takes only the index of the largest logit from the
// 32000, and the exact largest can be found from a per-row-scaled int8 copy of wcls (half the bytes) plus the fp16 rows of the few rows that can still win.
//   screen  (cls_screen_kernel): streams the int8 copy with cls_strip_body's ring, x chain and dealing of rows (gemv_strip_cls.h); per row r an approximate
//           logit A_r and a radius B_r with |A_r - L_r| <= B_r, L_r being the fp16 logit cls_strip_kernel / q4_matmul_f16 would have written, bit for bit;
//           per block the maximum of A_r - B_r over its rows.
//   refine  (cls_refine_kernel): the same grid and ownership of rows. G = max of the per-block maxima <= max_r L_r. Row r is a candidate unless
//           A_r + B_r < G (written that way round: a NaN makes a candidate). A candidate's owning wave streams the fp16 row and multiplies in
//           cls_strip_body's order -- slots, four v_dot2c from zero, sum += acc, wave_sum, one rounding: L_r's bits --, every other row gets -inf.
//   argmax_kernel then runs unchanged. The true argmax row has A + B >= L_max >= G, so has every row tied with it: the lowest-index rule sees the same
//   winners with the same bits. All logits -inf or NaN: token 0 both ways. A loose bound costs time, never the token.
// No launch here waits for another block: blocks talk across the launch boundary only.
//
// The copy (cls_screen_build, once per model: the weights never change after load). Row r, fp16 weights w as real numbers:
//   s = max|w| / 127 (fp32; an all-zero row: s = 0, q = 0), q = clamp(rint(w / s), -127, 127), e = w - s q,
//   E = ||e||_2, W = max(||w||_2, s ||q||_2) (float64, rounded up), stored: q as sign-magnitude bytes, s 2^24, EW = E + gamma W.
// A byte's magnitude sits in the low mantissa bits of an fp16 denormal (m 2^-24, the way the int4 kernels place nibbles) with the sign in bit 15: exact,
// and its product with an fp16 x is exact in fp32, so the screening dot product carries accumulation error only. Bytes are stored so that the even
// bytes of a word are elements 4k, 4k + 1 and the odd bytes 4k + 2, 4k + 3: two masks give the two half2 that meet x's natural pairs.
//
// The radius. X >= ||x||_2 of the staged (normalised) fp16 x: fp32, inflated by 2^-10. Cauchy-Schwarz: |s (q . x) - w . x| <= E X, however spiky x is.
//   B = ((EW X) (1 + 2^-11) + 2^-11 |A| + 2^-24) (1 + 2^-20)
// EW X covers the quantisation (E X) and the fp32 accumulation of BOTH dot products (gamma W X); 2^-11 (|A| + EW X) >= 2^-11 |t| the final fp16
// rounding of the classifier's fp32 sum t (|t| <= |A| + EW X); 2^-24 its rounding below fp16's normal range; the last factor B's own fp32 arithmetic.
// gamma = 2^-23 times the fp32 roundings on the longest path from a product to the row's sum, the two kernels ADDED (each errs against its own exact
// dot product: |fl - exact| <= gamma_k ||a|| ||x||, and ||w||, s ||q|| <= W). A v_dot2c_f32_f16 counts three: it truncates (EXPERIMENTS #30), and 2^-23
// per rounding covers truncation.
//   classifier (cls_strip_body, NS <= 10 slots): 4 dot2c chained from zero = 12, NS times sum += acc <= 10, wave_sum 4 DPP steps + 2 = 6: 28
//   screen (NS / 2 <= 5 pieces): 8 dot2c chained from zero = 24, sum += acc <= 5, wave_sum 6, the product with s 2^24 (a power of two times s: one) = 36
// gamma = 64 2^-23 = 2^-17 (k 2^-23 / (1 - k 2^-23) <= 2^-17 (1 + 2^-16): inside EW's own rounding up by 10^-6).
// A row whose |A| + B reaches fp16's overflow range (not < 65504), or is NaN, gets B = +inf: always a candidate, -inf to its block's maximum.
#pragma once
#include "q4_internal.h"

namespace q4 {

constexpr double CLS_SCREEN_GAMMA = 64.0 / 8388608.0;
enum { SCREEN_CUR = 0, SCREEN_OPEN = 1, SCREEN_LAST = 2, SCREEN_MAX = 3, SCREEN_TOTAL = 4, SCREEN_STEPS = 6, SCREEN_WORDS = 8 };   // TOTAL, STEPS: 64 bit

// a model's screening copy: ONE allocation (base), carved
struct ClsScreen {
    void* base = nullptr;
    unsigned char* q8 = nullptr;   // [d][n] sign-magnitude bytes
    float* scale = nullptr;        // [d] s_r 2^24
    float* ew = nullptr;           // [d] E_r + gamma W_r, rounded up
    float2* ab = nullptr;          // [d] (A_r, B_r) of the step
    float* lo = nullptr;           // [blocks] maximum of A_r - B_r over the block's rows
    q4_half* xn = nullptr;         // [n] the staged x of the step (behind the final norm)
    unsigned* count = nullptr;     // [SCREEN_WORDS] candidates: the step in progress, and the tallies the screen launch of the next step closes
    int n = 0, d = 0, blocks = 0;
};
bool cls_screen_shape(int n, int d);                                   // the strips form would admit the classifier (cls_strip_covers) and a wave's rows fit its lanes
int cls_screen_prepare();                                              // LDS opt-in, outside any capture
int cls_screen_build(ClsScreen* sc, const q4_half* wcls, int n, int d);   // Q4_ERR_ALLOC leaves *sc empty: the caller goes on without screening
void cls_screen_free(ClsScreen* sc);
// logits = L_r on candidate rows, -inf elsewhere (x itself is left as it is). rms_w null: x is taken as it is
int launch_cls_screen(const ClsScreen& sc, q4_half* logits, const q4_half* x, const q4_half* rms_w, const q4_half* wcls);
extern int g_greedy_screen;

}  // namespace q4
