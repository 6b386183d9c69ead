"""Poison for the fp16 K / V caches of a built Transformer (tests/test_stale_rows_gpu.py): rows [first_row, seq_len) of every layer of both caches are
overwritten through q4_memcpy_h2d on RunState::key_cache / value_cache, whose layout is [layer][seq_len][kv_dim] halves. The caches are zeroed when the
model is built and never by a generation, so what is written here stays until a step or a pass writes the row. The values are ordinary data: a kernel
that loads them faults nowhere -- it only computes with them."""
import numpy as np

NAN, MAX, MIN, INF = 0x7E00, 0x7BFF, 0xFBFF, 0x7C00
PATTERNS = ("nan", "huge")
CACHES = ("key_cache", "value_cache")


def pattern_row(pattern, kv_dim):
    """one row of the pattern, as uint16: nan -- every half a quiet NaN; huge -- +65504 / -65504 alternating, +inf at every 7th half"""
    if pattern == "nan":
        return np.full(kv_dim, NAN, dtype=np.uint16)
    assert pattern == "huge", pattern
    i = np.arange(kv_dim)
    return np.where(i % 7 == 6, INF, np.where(i % 2 == 0, MAX, MIN)).astype(np.uint16)


def _shape(t):
    cfg = t.config
    return cfg.n_layers, cfg.seq_len, cfg.dim * cfg.n_kv_heads // cfg.n_heads


def _row_address(t, cache, layer, row):
    _, seq_len, kv_dim = _shape(t)
    return getattr(t.state.contents, cache) + (layer * seq_len + row) * kv_dim * 2


def poison(q4, t, first_row, pattern, caches=CACHES):
    """rows [first_row, seq_len) of every layer of `caches` (both by default) become the pattern"""
    L = q4.lib()
    n_layers, seq_len, kv_dim = _shape(t)
    assert 0 <= first_row < seq_len and t.kv_format == "fp16"
    block = np.ascontiguousarray(np.tile(pattern_row(pattern, kv_dim), (seq_len - first_row, 1)))
    q4.check(L.q4_stream_synchronize())
    for cache in caches:
        for layer in range(n_layers):
            q4.check(L.q4_memcpy_h2d(_row_address(t, cache, layer, first_row), block.ctypes.data, block.nbytes))
    q4.check(L.q4_stream_synchronize())


def read_rows(q4, t, first_row, n_rows):
    """(K, V) rows [first_row, first_row + n_rows) of every layer as the cache holds them: uint16 [layers, n_rows, kv_dim] each"""
    L = q4.lib()
    n_layers, seq_len, kv_dim = _shape(t)
    assert 0 <= first_row and n_rows >= 0 and first_row + n_rows <= seq_len and t.kv_format == "fp16"
    out = [np.empty((n_layers, n_rows, kv_dim), dtype=np.uint16) for _ in CACHES]
    q4.check(L.q4_stream_synchronize())
    if n_rows:
        for dst, cache in zip(out, CACHES):
            for layer in range(n_layers):
                q4.check(L.q4_memcpy_d2h(dst[layer].ctypes.data, _row_address(t, cache, layer, first_row), dst[layer].nbytes))
    return out[0], out[1]


def assert_untouched(q4, t, first_row, pattern, what=""):
    """every byte of rows [first_row, seq_len) of both caches is still the pattern: nothing wrote there"""
    n_layers, seq_len, kv_dim = _shape(t)
    want = pattern_row(pattern, kv_dim)
    for name, rows in zip(CACHES, read_rows(q4, t, first_row, seq_len - first_row)):
        bad = np.argwhere((rows != want).any(axis=2))
        assert bad.size == 0, "%s: %s rows written above row %d: (layer, row) %s" % (what, name, first_row, [(int(a), int(b) + first_row) for a, b in bad[:8]])


def finite(u16):
    """True where every half of a uint16 array is finite"""
    return bool(((np.asarray(u16) & 0x7C00) != 0x7C00).all())
