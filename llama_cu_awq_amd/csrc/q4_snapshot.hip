// q4_snapshot.hip -- sequence snapshots: the K / V rows of a prefix kept beside the model, put back later or into another model of the same
// checkpoint, and their serialised form. Not in the reference.
// A snapshot holds positions [0, n_pos) packed on the device, in the cache's own element type (fp16 halves, or e4m3 bytes):
//   K rows [layer][n_pos][kv_dim], V rows [layer][n_pos][kv_dim]; an FP8 model's also K exponents [layer][n_kv_heads][n_pos], V exponents the same
// -- in this order, without padding: the buffer IS the blob's payload. The prefix of a layer is ONE contiguous run of the cache (n_pos * kv_dim elements
// out of seq_len * kv_dim), the exponents of a (layer, kv head) one run of n_pos bytes out of seq_len: taking and restoring a snapshot is one launch of
// q4_kv_copy.hip over two or four table entries. The snapshot does NOT hold: the FP8 staging rows (they are the current position's, not part of a
// prefix), logits, log-probability records, the guide's states, the sampler. It is immutable.
// The blob, little-endian: a 48-byte header {u32 magic "Q4SN", u32 version 1, i32 kv_format, i32 n_layers, i32 n_kv_heads, i32 head_size, i32 n_pos,
// f32 rope_theta, u64 fingerprint, u64 payload_bytes}, n_pos i32 tokens, the payload. q4_snapshot_check accepts a blob only when every count is in
// range and `bytes` is exactly what the header implies, computed in 64 bits with overflow checks before anything is allocated.
// fingerprint is Model::fingerprint: the checkpoint file's, and for a model with RoPE scaling that mixed with the fp32 bits of its frequencies (q4_model.hip) --
// rows rotated by other frequencies are refused by the same comparison, the header stays version 1.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include <new>
#include <vector>
#include "q4_model.h"
#include "q4_batch.h"
using namespace q4;

using SnapInfo = struct q4_snapshot_info;     // (the C ABI gives the record and the function that fills it one name: the tag needs its keyword)

struct q4_snapshot {
    void* dev;                   // the packed rows
    SnapInfo info;
    std::vector<int> tokens;     // [n_pos]
};

namespace {

enum : uint32_t { SNAP_MAGIC = 0x4E533451u, SNAP_VERSION = 1 };     // "Q4SN"
enum { SNAP_HEADER = 48, SNAP_MAX_COUNT = 1 << 16 };                // layers, kv heads, head size: far above any model, small enough that no product below overflows by accident

struct Layout {
    size_t kv_section;           // bytes of the K rows (= of the V rows)
    size_t exp_section;          // bytes of the K exponents (= of the V exponents), 0 for fp16
    size_t payload, blob;
};

// every size of a snapshot of these counts, or false: a count out of range or a size that does not fit 63 bits
bool layout_of(int kv_format, int n_layers, int n_kv_heads, int head_size, int n_pos, Layout* out) {
    if (kv_format != Q4_KV_FP16 && kv_format != Q4_KV_FP8) return false;
    if (n_layers < 1 || n_layers > SNAP_MAX_COUNT || n_kv_heads < 1 || n_kv_heads > SNAP_MAX_COUNT || head_size < 1 || head_size > SNAP_MAX_COUNT ||
        n_pos < 1 || n_pos > Q4_MAX_SEQ_LEN)
        return false;
    long long kv = kv_format == Q4_KV_FP8 ? 1 : (long long)sizeof(q4_half), ex = 0, payload, blob;
    if (__builtin_mul_overflow(kv, (long long)n_layers, &kv) || __builtin_mul_overflow(kv, (long long)n_pos, &kv) ||
        __builtin_mul_overflow(kv, (long long)n_kv_heads, &kv) || __builtin_mul_overflow(kv, (long long)head_size, &kv))
        return false;
    if (kv_format == Q4_KV_FP8) ex = (long long)n_layers * n_kv_heads * n_pos;       // (<= 2^16 * 2^16 * 2^17)
    if (__builtin_add_overflow(kv, ex, &payload) || __builtin_mul_overflow(payload, 2ll, &payload)) return false;
    if (__builtin_add_overflow(payload, (long long)SNAP_HEADER + 4ll * n_pos, &blob)) return false;
    out->kv_section = (size_t)kv; out->exp_section = (size_t)ex; out->payload = (size_t)payload; out->blob = (size_t)blob;
    return true;
}

template <class T> T rd(const unsigned char* p) { T v; memcpy(&v, p, sizeof(v)); return v; }      // (the hosts of this library are little-endian)
template <class T> void wr(unsigned char* p, T v) { memcpy(p, &v, sizeof(v)); }

// the table of one launch: dir 0 cache -> packed, 1 packed -> cache
int copy_rows(const Transformer* t, const Model* m, void* packed, const Layout& lay, int n_pos, int dir) {
    const Config* p = &t->config;
    const long long kv_dim = (long long)(p->dim / p->n_heads) * p->n_kv_heads, elem = m->kv_format == Q4_KV_FP8 ? 1 : (long long)sizeof(q4_half);
    const long long run = (long long)n_pos * kv_dim * elem, layer = (long long)p->seq_len * kv_dim * elem;
    char* base = (char*)packed;
    struct { void* cache; char* pack; long long outer, cache_stride, run_bytes; } part[KV_COPY_MAX_RUNS] = {
        {t->state.key_cache, base, p->n_layers, layer, run},
        {t->state.value_cache, base + lay.kv_section, p->n_layers, layer, run},
        {m->k_exp, base + 2 * lay.kv_section, (long long)p->n_layers * p->n_kv_heads, p->seq_len, n_pos},
        {m->v_exp, base + 2 * lay.kv_section + lay.exp_section, (long long)p->n_layers * p->n_kv_heads, p->seq_len, n_pos},
    };
    const int n = m->kv_format == Q4_KV_FP8 ? 4 : 2;
    CopyRun runs[KV_COPY_MAX_RUNS];
    for (int i = 0; i < n; i++) {
        if (!part[i].cache) return Q4_ERR_ARG;
        runs[i] = dir == 0 ? CopyRun{part[i].pack, part[i].cache, part[i].outer, part[i].run_bytes, part[i].cache_stride, part[i].run_bytes}
                           : CopyRun{part[i].cache, part[i].pack, part[i].outer, part[i].cache_stride, part[i].run_bytes, part[i].run_bytes};
    }
    return launch_copy_runs(runs, n);
}

int check_blob(const void* host, size_t bytes, SnapInfo* out, Layout* lay) {
    if (!host || bytes < SNAP_HEADER) return Q4_ERR_ARG;
    const unsigned char* h = (const unsigned char*)host;
    if (rd<uint32_t>(h) != SNAP_MAGIC || rd<uint32_t>(h + 4) != SNAP_VERSION) return Q4_ERR_ARG;
    SnapInfo info = {};
    info.kv_format = rd<int32_t>(h + 8);
    info.n_layers = rd<int32_t>(h + 12);
    info.n_kv_heads = rd<int32_t>(h + 16);
    info.head_size = rd<int32_t>(h + 20);
    info.n_pos = rd<int32_t>(h + 24);
    info.rope_theta = rd<float>(h + 28);
    info.fingerprint = rd<uint64_t>(h + 32);
    if (!layout_of(info.kv_format, info.n_layers, info.n_kv_heads, info.head_size, info.n_pos, lay)) return Q4_ERR_ARG;
    if (!isfinite(info.rope_theta) || rd<uint64_t>(h + 40) != (uint64_t)lay->payload || bytes != lay->blob) return Q4_ERR_ARG;
    info.device_bytes = lay->payload;
    info.export_bytes = lay->blob;
    if (out) *out = info;
    return Q4_OK;
}

}  // namespace

// what q4_batch_restore (q4_batch.hip) reads of a snapshot
const void* q4::snapshot_rows(const q4_snapshot* s) { return s->dev; }
const int* q4::snapshot_token_ids(const q4_snapshot* s) { return s->tokens.data(); }

extern "C" {

int q4_snapshot_new(q4_snapshot** out, const Transformer* t, int n_pos) {
    const Model* m = t ? model_of(&t->state) : nullptr;
    if (!out || !m) return Q4_ERR_ARG;
    Q4_HIP(hipStreamSynchronize(g_stream));
    const Config* p = &t->config;
    Layout lay;
    if (m->rows_suspect || n_pos < 1 || n_pos > t->state.shared_data->pos || n_pos > p->seq_len ||
        !layout_of(m->kv_format, p->n_layers, p->n_kv_heads, p->dim / p->n_heads, n_pos, &lay))
        return Q4_ERR_ARG;
    q4_snapshot* s = new (std::nothrow) q4_snapshot();
    if (!s) return Q4_ERR_ALLOC;
    if (hipMalloc(&s->dev, lay.payload) != hipSuccess) { (void)hipGetLastError(); delete s; return Q4_ERR_ALLOC; }
    s->info = SnapInfo{n_pos, m->kv_format, p->n_layers, p->n_kv_heads, p->dim / p->n_heads, p->rope_theta, m->fingerprint, lay.payload, lay.blob};
    s->tokens.assign(t->state.shared_data->tokens, t->state.shared_data->tokens + n_pos);
    int rc = copy_rows(t, m, s->dev, lay, n_pos, 0);
    if (!rc && hipStreamSynchronize(g_stream) != hipSuccess) rc = Q4_ERR_HIP;       // the rows are the snapshot's before the caller's next step overwrites them
    if (rc) { (void)hipFree(s->dev); delete s; return rc; }
    *out = s;
    return Q4_OK;
}

int q4_snapshot_restore(Transformer* t, const q4_snapshot* s) {
    const Model* m = t ? model_of(&t->state) : nullptr;
    if (!m || !s) return Q4_ERR_ARG;
    const Config* p = &t->config;
    const SnapInfo& i = s->info;
    if (i.fingerprint != m->fingerprint || i.kv_format != m->kv_format || i.n_layers != p->n_layers || i.n_kv_heads != p->n_kv_heads ||
        i.head_size != p->dim / p->n_heads || i.rope_theta != p->rope_theta || i.n_pos > p->seq_len)
        return Q4_ERR_ARG;
    Layout lay;
    if (!layout_of(i.kv_format, i.n_layers, i.n_kv_heads, i.head_size, i.n_pos, &lay)) return Q4_ERR_ARG;
    return copy_rows(t, m, s->dev, lay, i.n_pos, 1);
}

int q4_snapshot_delete(q4_snapshot* s) {
    if (!s) return Q4_ERR_ARG;
    if (g_stream) Q4_HIP(hipStreamSynchronize(g_stream));     // a restore may still read the rows
    if (s->dev) Q4_HIP(hipFree(s->dev));
    delete s;
    return Q4_OK;
}

int q4_snapshot_info(const q4_snapshot* s, struct q4_snapshot_info* out) {
    if (!s || !out) return Q4_ERR_ARG;
    *out = s->info;
    return Q4_OK;
}

int q4_snapshot_tokens(const q4_snapshot* s, int* out) {
    if (!s || !out) return Q4_ERR_ARG;
    memcpy(out, s->tokens.data(), s->tokens.size() * sizeof(int));
    return Q4_OK;
}

int q4_snapshot_check(const void* host, size_t bytes, struct q4_snapshot_info* out) {
    Layout lay;
    return check_blob(host, bytes, out, &lay);
}

int q4_snapshot_export(const q4_snapshot* s, void* host, size_t capacity) {
    if (!s || !host || capacity < s->info.export_bytes) return Q4_ERR_ARG;
    unsigned char* h = (unsigned char*)host;
    const SnapInfo& i = s->info;
    wr<uint32_t>(h, SNAP_MAGIC); wr<uint32_t>(h + 4, SNAP_VERSION);
    wr<int32_t>(h + 8, i.kv_format); wr<int32_t>(h + 12, i.n_layers); wr<int32_t>(h + 16, i.n_kv_heads); wr<int32_t>(h + 20, i.head_size);
    wr<int32_t>(h + 24, i.n_pos); wr<float>(h + 28, i.rope_theta); wr<uint64_t>(h + 32, i.fingerprint); wr<uint64_t>(h + 40, i.device_bytes);
    memcpy(h + SNAP_HEADER, s->tokens.data(), (size_t)i.n_pos * sizeof(int));
    if (g_stream) Q4_HIP(hipStreamSynchronize(g_stream));
    Q4_HIP(hipMemcpy(h + SNAP_HEADER + (size_t)i.n_pos * sizeof(int), s->dev, i.device_bytes, hipMemcpyDeviceToHost));
    return Q4_OK;
}

int q4_snapshot_import(q4_snapshot** out, const void* host, size_t bytes) {
    if (!out) return Q4_ERR_ARG;
    SnapInfo info;
    Layout lay;
    Q4_TRY(check_blob(host, bytes, &info, &lay));
    q4_snapshot* s = new (std::nothrow) q4_snapshot();
    if (!s) return Q4_ERR_ALLOC;
    if (hipMalloc(&s->dev, lay.payload) != hipSuccess) { (void)hipGetLastError(); delete s; return Q4_ERR_ALLOC; }
    const unsigned char* h = (const unsigned char*)host;
    s->info = info;
    s->tokens.resize(info.n_pos);
    memcpy(s->tokens.data(), h + SNAP_HEADER, (size_t)info.n_pos * sizeof(int));
    if (hipMemcpy(s->dev, h + SNAP_HEADER + (size_t)info.n_pos * sizeof(int), lay.payload, hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipGetLastError();
        (void)hipFree(s->dev);
        delete s;
        return Q4_ERR_HIP;
    }
    *out = s;
    return Q4_OK;
}

}  // extern "C"
