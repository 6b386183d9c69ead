"""q4_kv_shift, the context shift's launch (csrc/q4_kv_shift.hip), op-level and BIT FOR BIT against the numpy restatement (context_shift_ref): buffers
filled from a seed, every byte that must not change compared with what it held -- rows below n_keep, rows at or above n_pos, their exponent bytes, and
guard bytes around every allocation. The rotation table is the test's own float32 array, so numpy computes with the bits the kernel reads."""
import numpy as np
import pytest

import context_shift_ref as ref
import kv8_ref

pytestmark = pytest.mark.gpu
ERR_ARG = 5
U = 16                       # KS_U in csrc/q4_kv_shift.hip: the rows a work item keeps in flight
GUARD = 64                   # bytes in front of and behind every buffer (a multiple of 16: the buffers stay aligned)
LAYERS, HEADS, SEQ = 2, 2, 77          # rows of 77 positions: neither the rows' nor the exponent runs' extent is a multiple of 16 bytes
# (n_pos, keep, D): maximal overlap (D = 1), M just above and just below D, M = 0, keep = 0, n_pos below seq_len
POSITIONS = [(77, 0, 1), (77, 4, 1), (77, 4, 36), (77, 4, 37), (77, 4, 73), (40, 0, 40), (9, 3, 2)]
# every M from 0 to 2 U + 1 at D = 1 and D = 3: the prologue alone, one slot short of a round, a round and a bit
WALKS = [(2 + D + M, 2, D) for D in (1, 3) for M in range(2 * U + 2)]


class Guarded:
    """a device buffer holding `arr` between two guards"""

    def __init__(self, q4, arr):
        self.q4, self.shape, self.dtype = q4, arr.shape, arr.dtype
        raw = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
        self.n = raw.size
        self.buf = q4.DevBuf(np.concatenate([np.full(GUARD, 0xA5, np.uint8), raw, np.full(GUARD, 0x5A, np.uint8)]))
        self.ptr = self.buf.ptr + GUARD

    def get(self):
        raw = self.buf.get(np.uint8, self.n + 2 * GUARD)
        assert (raw[:GUARD] == 0xA5).all() and (raw[GUARD + self.n:] == 0x5A).all(), "a guard byte changed"
        return raw[GUARD:GUARD + self.n].view(self.dtype).reshape(self.shape)


def table_for(D, head_size, theta=1e4):
    return np.ascontiguousarray(ref.rope_table_row(D, head_size, theta), dtype=np.float32)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint16 if a.dtype == np.float16 else np.uint8)


def check_fp16(q4, k, v, head_size, n_pos, keep, D, seq=SEQ, heads=HEADS):
    """one launch over copies of k and v [layers, seq, kv_dim]; everything but rows [n_pos - D, n_pos) must equal the restatement's"""
    table = table_for(D, head_size)
    gk, gv, gt = Guarded(q4, k), Guarded(q4, v), Guarded(q4, table)
    q4.check(q4.lib().q4_kv_shift(gk.ptr, gv.ptr, None, None, q4.KV_FP16, k.shape[0], seq, heads, head_size, n_pos, keep, D, gt.ptr))
    q4.synchronize()
    wk, wv = k.copy(), v.copy()
    ref.shift_fp16(wk, wv, n_pos, keep, D, head_size, table)
    ok, ov = gk.get(), gv.get()
    gt.get()
    what = "head_size %d (n_pos, keep, D) = (%d, %d, %d)" % (head_size, n_pos, keep, D)
    for got, want, name in ((ok, wk, "K"), (ov, wv, "V")):
        for lo, hi in ((0, n_pos - D), (n_pos, seq)):
            assert np.array_equal(bits(got[:, lo:hi]), bits(want[:, lo:hi])), "%s rows [%d, %d): %s" % (name, lo, hi, what)
    assert np.array_equal(bits(ov[:, keep:n_pos - D]), bits(v[:, keep + D:n_pos])), what           # V: the moved input itself
    assert np.array_equal(bits(ok[:, :keep]), bits(k[:, :keep])) and np.array_equal(bits(ok[:, n_pos:]), bits(k[:, n_pos:])), what


def random_rows(rng, head_size, seq=SEQ, heads=HEADS, layers=LAYERS):
    shape = (layers, seq, heads * head_size)
    scale = 10.0 ** rng.integers(-4, 3, size=(layers, seq, 1))                  # mixed scales from row to row
    return (rng.standard_normal(shape) * scale).astype(np.float16), rng.standard_normal(shape).astype(np.float16)


@pytest.mark.parametrize("head_size", [32, 64, 80, 96, 128, 256, 34])
def test_fp16_rows_move_and_k_rotates(q4, head_size):
    """head sizes with 16-byte chunk pairs, and 34: the scalar kernel"""
    rng = np.random.default_rng(head_size)
    k, v = random_rows(rng, head_size)
    for n_pos, keep, D in POSITIONS:
        check_fp16(q4, k, v, head_size, n_pos, keep, D)


@pytest.mark.parametrize("head_size", [64, 34])
def test_fp16_every_fill_of_the_load_ring(q4, head_size):
    rng = np.random.default_rng(7 + head_size)
    k, v = random_rows(rng, head_size)
    for n_pos, keep, D in WALKS:
        check_fp16(q4, k, v, head_size, n_pos, keep, D)


def test_fp16_more_work_items_than_one_grid_pass(q4):
    """80 layers x 64 kv heads of 256: 2 x 1280 units of 64 items, more than the eight blocks per CU the grid is sized to, so the blocks stride"""
    rng = np.random.default_rng(99)
    k = rng.standard_normal((80, 6, 64 * 256)).astype(np.float16)
    v = rng.standard_normal((80, 6, 64 * 256)).astype(np.float16)
    check_fp16(q4, k, v, 256, 6, 1, 2, seq=6, heads=64)


@pytest.mark.parametrize("head_size", [64, 34])
def test_fp16_hostile_values(q4, head_size):
    """+-65504 (a rotated pair may round to +-inf: the IEEE result is the specification, and numpy agrees), subnormals, +-0, mixed scales"""
    rng = np.random.default_rng(11)
    k, v = random_rows(rng, head_size)
    flat = k.reshape(-1)
    n = flat.size
    flat[rng.integers(0, n, n // 4)] = np.float16(65504)
    flat[rng.integers(0, n, n // 4)] = np.float16(-65504)
    flat[rng.integers(0, n, n // 8)] = np.float16(0.0)
    flat[rng.integers(0, n, n // 8)] = np.float16(-0.0)
    sub = rng.integers(1, 1024, n // 8).astype(np.uint16) | (rng.integers(0, 2, n // 8).astype(np.uint16) << 15)
    flat[rng.integers(0, n, n // 8)] = sub.view(np.float16)
    k[:, 50:60] = np.float16(65504)                                               # whole rows at the largest half
    k[:, 60:64] = np.float16(-65504)
    assert not np.isnan(k.astype(np.float32)).any()
    for n_pos, keep, D in [(77, 4, 1), (77, 4, 36), (77, 0, 5)]:
        check_fp16(q4, k, v, head_size, n_pos, keep, D)
    table = table_for(5, head_size)
    assert np.isinf(ref.rotate(k[:, 50:64], head_size, table).astype(np.float32)).any()          # (the case does occur)


# ---- FP8 -----------------------------------------------------------------------------------------------------------------------------------------------
E4M3_448, E4M3_320, E4M3_240 = 0x7E, 0x7A, 0x77          # 1.75 * 2^8, 1.25 * 2^8, 1.875 * 2^7


def fp8_rows(rng, head_size, D):
    """random bytes (no NaN code) and exponents across [-15, 7]; then rows built to make the rotated amax cross a power of two both ways (one pair
    (x, x) near 448 * 2^e / sqrt 2 where cos + sin is largest: up; one pair (240, 0) where the angle is nearest 45 degrees: down), all-zero rows, rows
    at +-448 * 2^7"""
    shape = (LAYERS, SEQ, HEADS * head_size)
    k = rng.integers(0, 256, shape, dtype=np.uint8)
    v = rng.integers(0, 256, shape, dtype=np.uint8)
    for a in (k, v):
        a[(a & 0x7F) == 0x7F] = 0x38
    ke = rng.integers(kv8_ref.E_MIN, kv8_ref.E_MAX + 1, (LAYERS, HEADS, SEQ)).astype(np.int8)
    ve = rng.integers(kv8_ref.E_MIN, kv8_ref.E_MAX + 1, (LAYERS, HEADS, SEQ)).astype(np.int8)
    table = table_for(D, head_size).astype(np.float64)
    hp = head_size // 2
    c, s = table[:, 0], table[:, 1]
    up = int(np.argmax(np.maximum(np.abs(c + s), np.abs(c - s))))
    down = int(np.argmin(np.abs(np.abs(c) - np.abs(s))))
    rows = k.reshape(LAYERS, SEQ, HEADS, head_size)
    rows[:, 20:24] = 0
    rows[:, 20:24, :, up] = E4M3_320
    rows[:, 20:24, :, up + hp] = E4M3_320
    rows[:, 24:28] = 0
    rows[:, 24:28, :, down] = E4M3_240
    rows[:, 28:30] = 0                                                             # all-zero rows (+0), and -0
    rows[:, 30:32] = 0x80
    rows[:, 32:34] = E4M3_448
    rows[:, 34:36] = E4M3_448 | 0x80
    ke[:, :, 32:36] = 7
    ke[:, :, 20:22] = -15                                                          # ... at both ends of the exponent range too
    ke[:, :, 26:28] = 7
    return k, v, ke, ve


def check_fp8(q4, k, v, ke, ve, head_size, n_pos, keep, D):
    table = table_for(D, head_size)
    g = [Guarded(q4, a) for a in (k, v, ke, ve, table)]
    q4.check(q4.lib().q4_kv_shift(g[0].ptr, g[1].ptr, g[2].ptr, g[3].ptr, q4.KV_FP8, LAYERS, SEQ, HEADS, head_size, n_pos, keep, D, g[4].ptr))
    q4.synchronize()
    want = [a.copy() for a in (k, v, ke, ve)]
    ref.shift_fp8(*want, n_pos, keep, D, head_size, table)
    got = [x.get() for x in g[:4]]
    g[4].get()
    what = "head_size %d (n_pos, keep, D) = (%d, %d, %d)" % (head_size, n_pos, keep, D)
    for lo, hi in ((0, n_pos - D), (n_pos, SEQ)):
        for i, name in ((0, "K bytes"), (1, "V bytes")):
            assert np.array_equal(got[i][:, lo:hi], want[i][:, lo:hi]), "%s rows [%d, %d): %s" % (name, lo, hi, what)
        for i, name in ((2, "K exponents"), (3, "V exponents")):
            assert np.array_equal(got[i][:, :, lo:hi], want[i][:, :, lo:hi]), "%s [%d, %d): %s" % (name, lo, hi, what)
    assert np.array_equal(got[1][:, keep:n_pos - D], v[:, keep + D:n_pos]) and np.array_equal(got[3][:, :, keep:n_pos - D], ve[:, :, keep + D:n_pos]), what
    moved_old, moved_new = ke[:, :, keep + D:n_pos].astype(int), want[2][:, :, keep:n_pos - D].astype(int)
    return bool((moved_new > moved_old).any()), bool((moved_new < moved_old).any())


@pytest.mark.parametrize("head_size", [64, 128, 256])
def test_fp8_rows_move_and_k_is_requantised(q4, head_size):
    rng = np.random.default_rng(1000 + head_size)
    went_up = went_down = False
    for n_pos, keep, D in POSITIONS:
        k, v, ke, ve = fp8_rows(rng, head_size, D)
        up, down = check_fp8(q4, k, v, ke, ve, head_size, n_pos, keep, D)
        went_up, went_down = went_up or up, went_down or down
    assert went_up and went_down                                                   # the exponent did change in both directions


def test_fp8_every_fill_of_the_load_ring(q4):
    rng = np.random.default_rng(17)
    for n_pos, keep, D in WALKS:
        k, v, ke, ve = fp8_rows(rng, 128, D)
        check_fp8(q4, k, v, ke, ve, 128, n_pos, keep, D)


def test_fp8_built_rows_cross_a_power_of_two(q4):
    """the rows built by fp8_rows, moved with D = 1 from where they sit: the exponent rises for the (x, x) rows and falls for the (240, 0) rows"""
    rng = np.random.default_rng(3)
    k, v, ke, ve = fp8_rows(rng, 64, 1)
    ke[:, :, 22:26] = 0
    table = table_for(1, 64)
    want = [a.copy() for a in (k, v, ke, ve)]
    ref.shift_fp8(*want, 77, 0, 1, 64, table)
    assert (want[2][:, :, 21:23] == 1).all() and (want[2][:, :, 23:25] == -1).all()
    check_fp8(q4, k, v, ke, ve, 64, 77, 0, 1)


# ---- refusals, and the launch that has nothing to move --------------------------------------------------------------------------------------------------
def test_no_discard_is_refused_and_no_row_to_move_writes_nothing(q4):
    rng = np.random.default_rng(21)
    k, v = random_rows(rng, 64)
    table = table_for(3, 64)
    gk, gv, gt = Guarded(q4, k), Guarded(q4, v), Guarded(q4, table)
    L = q4.lib()
    assert L.q4_kv_shift(gk.ptr, gv.ptr, None, None, q4.KV_FP16, LAYERS, SEQ, HEADS, 64, 77, 4, 0, gt.ptr) == ERR_ARG          # D = 0
    assert L.q4_kv_shift(gk.ptr, gv.ptr, None, None, q4.KV_FP16, LAYERS, SEQ, HEADS, 64, 78, 4, 3, gt.ptr) == ERR_ARG          # n_pos above seq_len
    assert L.q4_kv_shift(gk.ptr, gv.ptr, None, None, q4.KV_FP16, LAYERS, SEQ, HEADS, 64, 6, 4, 3, gt.ptr) == ERR_ARG           # keep + D > n_pos
    assert L.q4_kv_shift(gk.ptr, gv.ptr, None, None, q4.KV_FP8, LAYERS, SEQ, HEADS, 64, 77, 4, 3, gt.ptr) == ERR_ARG           # FP8 without exponents
    q4.check(L.q4_kv_shift(gk.ptr, gv.ptr, None, None, q4.KV_FP16, LAYERS, SEQ, HEADS, 64, 7, 4, 3, gt.ptr))                   # n_pos = keep + D: M = 0
    q4.synchronize()
    assert np.array_equal(bits(gk.get()), bits(k)) and np.array_equal(bits(gv.get()), bits(v))
