// q4_kv_copy.hip -- one launch that copies a small table of strided runs, device to device: what moves the K / V rows (and, for an FP8 cache, the row
// exponents) of a prefix between a model's caches and a snapshot's packed buffer (q4_snapshot.hip). Not in the reference.
// A table entry is {dst, src, outer, dst_stride, src_stride, run_bytes}: run r of an entry copies run_bytes bytes from src + r * src_stride to
// dst + r * dst_stride, r < outer. At most KV_COPY_MAX_RUNS entries per launch (K, V, K exponents, V exponents); the table travels by value in the
// kernel's arguments, so the launch allocates nothing, copies nothing from the host and is safe to capture.
// Work: every run is cut into pieces of KV_COPY_PIECE bytes; the pieces of all entries form one list, and the blocks of a grid sized from the stream's
// CU count (not from the byte count) walk it with a grid stride. Inside a run whose source and destination have the SAME offset from a 16-byte boundary,
// a head of up to 15 bytes brings both to the boundary, the body moves as 16-byte vectors -- non-temporal loads and stores: the bytes are used once, and
// a 1 GB prefix must not push the weights out of the Infinity Cache -- and a tail of up to 15 bytes follows. Heads, tails and every run whose two offsets
// differ (exponent runs start at multiples of seq_len, which need not be a multiple of 16) go byte by byte in plain C++. A thread requests its four
// vectors of a piece before it stores the first. Every offset is 64-bit (a layer offset passes 2^31 bytes at 13B x 16 K positions). No atomics, no
// ordering beyond the stream's: every destination byte is written by exactly one thread, once.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "q4_device.h"
#include "q4_model.h"
using namespace q4;

namespace {

constexpr int KC_T = 256, KC_Q = 4;                          // threads per block, 16-byte vectors per thread and piece
constexpr long long KC_VEC = (long long)KC_T * KC_Q;         // vectors per piece
constexpr long long KV_COPY_PIECE = KC_VEC * 16;             // 16 KiB
constexpr int KC_BLOCKS_PER_CU = 8;                          // 32 waves per CU: the memory system's queue depth, not arithmetic, is what a copy needs

struct CopyTable {
    CopyRun run[KV_COPY_MAX_RUNS];
    long long pieces_per_run[KV_COPY_MAX_RUNS];
    long long first_piece[KV_COPY_MAX_RUNS + 1];             // prefix sums: the entry's first piece in the launch's list
    int n;
};

__global__ void __launch_bounds__(KC_T) kv_copy_kernel(const CopyTable tab) {
    const int tid = threadIdx.x;
    const long long total = tab.first_piece[tab.n];
    for (long long u = blockIdx.x; u < total; u += gridDim.x) {
        int e = 0;
        while (e + 1 < tab.n && u >= tab.first_piece[e + 1]) e++;
        const CopyRun& cr = tab.run[e];
        const long long ppr = tab.pieces_per_run[e];
        const long long local = u - tab.first_piece[e];
        const long long r = local / ppr, piece = local - r * ppr;
        unsigned char* d = (unsigned char*)cr.dst + r * cr.dst_stride;
        const unsigned char* s = (const unsigned char*)cr.src + r * cr.src_stride;
        const long long n = cr.run_bytes;
        if ((((uintptr_t)d ^ (uintptr_t)s) & 15) != 0) {     // the two offsets differ: no 16-byte access can be aligned on both sides
            const long long b0 = piece * KV_COPY_PIECE, b1 = b0 + KV_COPY_PIECE < n ? b0 + KV_COPY_PIECE : n;
            for (long long i = b0 + tid; i < b1; i += KC_T) d[i] = s[i];
            continue;
        }
        long long head = (long long)((16 - ((uintptr_t)d & 15)) & 15);
        if (head > n) head = n;
        const long long nv = (n - head) >> 4;               // whole vectors behind the head; nv <= ppr * KC_VEC, so the pieces cover them
        if (piece == 0 && tid < head) d[tid] = s[tid];
        if (piece == ppr - 1) {
            const long long t0 = head + (nv << 4);
            if (t0 + tid < n) d[t0 + tid] = s[t0 + tid];
        }
        const u32x4* sv = (const u32x4*)(s + head);
        u32x4* dv = (u32x4*)(d + head);
        const long long v0 = piece * KC_VEC;
        u32x4 q[KC_Q];
#pragma unroll
        for (int k = 0; k < KC_Q; k++) {
            const long long v = v0 + tid + (long long)k * KC_T;
            if (v < nv) q[k] = __builtin_nontemporal_load(sv + v);
        }
#pragma unroll
        for (int k = 0; k < KC_Q; k++) {
            const long long v = v0 + tid + (long long)k * KC_T;
            if (v < nv) __builtin_nontemporal_store(q[k], dv + v);
        }
    }
}

// [a, a + span) of an entry's side: the bytes from its first run's first to its last run's last
bool span_of(const void* base, long long outer, long long stride, long long run_bytes, uintptr_t* lo, uintptr_t* hi) {
    long long reach;
    if (__builtin_mul_overflow(outer - 1, stride, &reach) || __builtin_add_overflow(reach, run_bytes, &reach)) return false;
    *lo = (uintptr_t)base;
    if (__builtin_add_overflow((uintptr_t)base, (uintptr_t)reach, hi)) return false;
    return true;
}

}  // namespace

namespace q4 {

int copy_runs_check(const CopyRun& c) {
    if (!c.dst || !c.src || c.outer < 0 || c.dst_stride < 0 || c.src_stride < 0 || c.run_bytes < 0) return Q4_ERR_ARG;
    if (c.outer == 0 || c.run_bytes == 0) return Q4_OK;
    if (c.outer > 1 && (c.run_bytes > c.dst_stride || c.run_bytes > c.src_stride)) return Q4_ERR_ARG;   // runs of one side would overlap each other
    uintptr_t d0, d1, s0, s1;
    if (!span_of(c.dst, c.outer, c.dst_stride, c.run_bytes, &d0, &d1) || !span_of(c.src, c.outer, c.src_stride, c.run_bytes, &s0, &s1)) return Q4_ERR_ARG;
    if (d0 < s1 && s0 < d1) return Q4_ERR_ARG;               // the two ranges overlap
    return Q4_OK;
}

int launch_copy_runs(const CopyRun* runs, int n) {
    if (!runs || n < 0 || n > KV_COPY_MAX_RUNS) return Q4_ERR_ARG;
    CopyTable tab = {};
    for (int i = 0; i < n; i++) {
        Q4_TRY(copy_runs_check(runs[i]));
        if (runs[i].outer == 0 || runs[i].run_bytes == 0) continue;
        const long long ppr = (runs[i].run_bytes + KV_COPY_PIECE - 1) / KV_COPY_PIECE;
        long long pieces;
        if (__builtin_mul_overflow(ppr, runs[i].outer, &pieces) || __builtin_add_overflow(tab.first_piece[tab.n], pieces, &pieces)) return Q4_ERR_ARG;
        tab.run[tab.n] = runs[i];
        tab.pieces_per_run[tab.n] = ppr;
        tab.first_piece[tab.n + 1] = pieces;
        tab.n++;
    }
    const long long total = tab.first_piece[tab.n];
    if (total == 0) return Q4_OK;
    const long long room = (long long)stream_cu_count() * KC_BLOCKS_PER_CU;
    const unsigned blocks = (unsigned)(total < room ? total : room);
    Q4_LAUNCH(kv_copy_kernel, dim3(blocks), dim3(KC_T), 0, tab);
    Q4_LAUNCH_CHECK();
    return Q4_OK;
}

}  // namespace q4

extern "C" int q4_copy_runs(void* dst, const void* src, long long outer, long long dst_stride, long long src_stride, long long run_bytes) {
    const CopyRun c = {dst, src, outer, dst_stride, src_stride, run_bytes};
    return launch_copy_runs(&c, 1);
}
