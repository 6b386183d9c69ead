"""q4_copy_runs (csrc/q4_kv_copy.hip), the launch that takes and restores snapshots, against numpy slicing: byte for byte, with a canary over every
byte of the destination that no run covers."""
import ctypes as C
import itertools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RUNS = (1, 15, 16, 17, 4096 + 5)      # below, at and above one vector; a piece and a tail
OUTER = (1, 3)
OFFSETS = (0, 4, 9)                   # of a base from a 16-byte boundary (allocations are aligned far beyond that)
PAD = 64                              # canary bytes kept in front of and behind everything a case touches
ERR_ARG = 5


def strides(run):
    """the packed form, and a stride that is no multiple of 16 (1300: an exponent row of synth's head64_long)"""
    return (run, 1300 if run <= 1300 else run + 1300)


def canary(n):
    return ((np.arange(n, dtype=np.uint32) * 31 + 7) % 253).astype(np.uint8)


@pytest.fixture(scope="module")
def bufs(q4):
    n = PAD + 16 + 3 * (4101 + 1300) + PAD
    rng = np.random.default_rng(99)
    src = rng.integers(0, 256, n, dtype=np.uint8)
    b = {"n": n, "src": src, "dsrc": q4.DevBuf(src), "ddst": q4.DevBuf(nbytes=n), "dthird": q4.DevBuf(nbytes=n)}
    yield b
    for k in ("dsrc", "ddst", "dthird"):
        b[k].free()


def expect(dst, src, doff, soff, outer, ds, ss, run):
    out = dst.copy()
    for r in range(outer):
        out[doff + r * ds: doff + r * ds + run] = src[soff + r * ss: soff + r * ss + run]
    return out


def cases():
    return itertools.product(RUNS, OUTER, OFFSETS, OFFSETS, (0, 1))


def test_pack_direction(q4, bufs):
    """strided source (a cache's layer stride), packed destination"""
    n, src = bufs["n"], bufs["src"]
    for run, outer, doff, soff, kind in cases():
        ss, ds = strides(run)[kind], run
        before = canary(n)
        bufs["ddst"].put(before)
        q4.copy_runs(bufs["ddst"], bufs["dsrc"], outer, ds, ss, run, dst_offset=PAD + doff, src_offset=PAD + soff)
        got = bufs["ddst"].get(np.uint8)[:n]
        want = expect(before, src, PAD + doff, PAD + soff, outer, ds, ss, run)
        assert np.array_equal(got, want), (run, outer, doff, soff, ss, int(np.argmax(got != want)))


def test_unpack_direction(q4, bufs):
    """packed source, strided destination: every byte between the runs keeps its canary"""
    n, src = bufs["n"], bufs["src"]
    for run, outer, doff, soff, kind in cases():
        ss, ds = run, strides(run)[kind]
        before = canary(n)
        bufs["ddst"].put(before)
        q4.copy_runs(bufs["ddst"], bufs["dsrc"], outer, ds, ss, run, dst_offset=PAD + doff, src_offset=PAD + soff)
        got = bufs["ddst"].get(np.uint8)[:n]
        want = expect(before, src, PAD + doff, PAD + soff, outer, ds, ss, run)
        assert np.array_equal(got, want), (run, outer, doff, soff, ds, int(np.argmax(got != want)))


def test_round_trip(q4, bufs):
    """pack, then unpack at another alignment in the same stream: the runs come back, nothing else moves"""
    n, src = bufs["n"], bufs["src"]
    for run, outer, doff, soff, kind in cases():
        big = strides(run)[kind]
        mid_before, end_before = canary(n), canary(n)[::-1].copy()
        bufs["ddst"].put(mid_before)
        bufs["dthird"].put(end_before)
        q4.copy_runs(bufs["ddst"], bufs["dsrc"], outer, run, big, run, dst_offset=PAD + doff, src_offset=PAD + soff)
        q4.copy_runs(bufs["dthird"], bufs["ddst"], outer, big, run, run, dst_offset=PAD + soff, src_offset=PAD + doff)
        mid = expect(mid_before, src, PAD + doff, PAD + soff, outer, run, big, run)
        want = expect(end_before, mid, PAD + soff, PAD + doff, outer, big, run, run)
        got = bufs["dthird"].get(np.uint8)[:n]
        assert np.array_equal(got, want), (run, outer, doff, soff, big)
        for r in range(outer):      # ... which is the source's runs where they were
            at = PAD + soff + r * big
            assert np.array_equal(got[at: at + run], src[at: at + run])


def test_more_pieces_than_one_block_takes(q4):
    """a run of several 16 KiB pieces with a head and a tail, more runs than one: the grid-stride walk over (run, piece)"""
    run, outer, stride = 5 * 16384 + 16 * 3 + 11, 7, 6 * 16384 + 20
    rng = np.random.default_rng(5)
    src = rng.integers(0, 256, PAD + outer * stride + PAD, dtype=np.uint8)
    n = PAD + outer * run + PAD
    dsrc, ddst = q4.DevBuf(src), q4.DevBuf(canary(n))
    q4.copy_runs(ddst, dsrc, outer, run, stride, run, dst_offset=PAD + 9, src_offset=PAD + 9 + 16)
    want = expect(canary(n), src, PAD + 9, PAD + 9 + 16, outer, run, stride, run)
    assert np.array_equal(ddst.get(np.uint8)[:n], want)
    dsrc.free()
    ddst.free()


def test_offsets_beyond_32_bits(q4):
    """outer 3, a source stride of 2^31 + 48 bytes, runs of 4 KiB: the third run starts past 2^32 (a layer offset at 13B x 16 K positions passes 2^31)"""
    L = q4.lib()
    stride, run, outer = (1 << 31) + 48, 4096, 3
    big = q4.DevBuf(nbytes=(outer - 1) * stride + run)          # needs no host array
    rng = np.random.default_rng(17)
    pieces = [rng.integers(0, 256, run, dtype=np.uint8) for _ in range(outer)]
    for r, p in enumerate(pieces):
        q4.check(L.q4_memcpy_h2d(big.ptr + r * stride, p.ctypes.data, run))
    n = PAD + outer * run + PAD
    dst = q4.DevBuf(canary(n))
    q4.copy_runs(dst, big, outer, run, stride, run, dst_offset=PAD)
    want = canary(n)
    want[PAD: PAD + outer * run] = np.concatenate(pieces)
    assert np.array_equal(dst.get(np.uint8)[:n], want)
    # ... and back, to the far ends of a second large buffer
    big2 = q4.DevBuf(nbytes=(outer - 1) * stride + run)
    q4.copy_runs(big2, dst, outer, stride, run, run, src_offset=PAD)
    for r, p in enumerate(pieces):
        back = np.empty(run, dtype=np.uint8)
        q4.check(L.q4_memcpy_d2h(back.ctypes.data, big2.ptr + r * stride, run))
        assert np.array_equal(back, p), r
    edge = np.empty(32, dtype=np.uint8)
    q4.check(L.q4_memcpy_d2h(edge.ctypes.data, big2.ptr + stride - 32, 32))      # (DevBuf zeroes what it allocates)
    assert not edge.any()
    for b in (big, big2, dst):
        b.free()


def test_refusals(q4):
    L = q4.lib()
    a, b = q4.DevBuf(nbytes=4096), q4.DevBuf(canary(4096))
    for args in ((-1, 16, 16, 16), (2, -16, 16, 16), (2, 16, -16, 16), (2, 16, 16, -1), (2, 15, 16, 16), (2, 16, 15, 16)):
        assert L.q4_copy_runs(a.ptr, b.ptr, *args) == ERR_ARG, args
    assert L.q4_copy_runs(a.ptr, a.ptr + 8, 1, 16, 16, 16) == ERR_ARG            # overlapping ranges
    assert L.q4_copy_runs(a.ptr + 100, a.ptr, 3, 40, 40, 30) == ERR_ARG
    assert L.q4_copy_runs(None, b.ptr, 1, 16, 16, 16) == ERR_ARG
    assert L.q4_copy_runs(a.ptr, None, 1, 16, 16, 16) == ERR_ARG
    assert L.q4_copy_runs(a.ptr, a.ptr + 16, 1, 16, 16, 16) == 0                 # adjacent is not overlapping
    q4.synchronize()
    assert not a.get(np.uint8)[:16].any() and np.array_equal(b.get(np.uint8), canary(4096))   # a refused call wrote nothing
    a.free()
    b.free()
