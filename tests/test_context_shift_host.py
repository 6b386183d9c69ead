"""Context shift without a GPU: the new symbols, the parser, the argument checks that run in front of any launch, and the numpy restatement
(context_shift_ref) against the oracle's own RoPE -- which pins the sign and pairing conventions of the rotation before any kernel runs."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import context_shift_ref as ref

ERR_ARG = 5
NEW = ["q4_shift_context", "q4_set_context_shift", "q4_get_context_shift", "q4_parse_context_shift", "q4_get_rope_row", "q4_kv_shift"]


def test_every_new_symbol_is_exported_and_listed():
    from llama_cu_awq_amd import api
    out = subprocess.check_output(["nm", "-D", "--defined-only", api.LIB_PATH]).decode()
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    for name in NEW:
        assert name in exported, name
        assert name in api.SYMBOLS, name
        assert getattr(api.lib(), name).argtypes is not None, name


def _parse(text):
    from llama_cu_awq_amd import api
    keep, discard = C.c_int(-7), C.c_int(-9)
    rc = api.lib().q4_parse_context_shift(text.encode(), C.byref(keep), C.byref(discard))
    return rc, keep.value, discard.value


def test_parse_round_trips():
    assert _parse("keep=4,discard=64") == (0, 4, 64)
    assert _parse("discard=64,keep=4") == (0, 4, 64)
    assert _parse("discard=8") == (0, 0, 8)
    assert _parse("keep=0,discard=1") == (0, 0, 1)


@pytest.mark.parametrize("text", ["", "keep=4", "discard=0", "keep=4,discard=0", "drop=3", "keep=4,discard=8,more=1", "discard=x", "discard=8x", "discard=",
                                  "=8", "discard=-8", "keep=-1,discard=8", "discard=8,", ",discard=8", "discard= 8", "discard=+8", "discard=8.5",
                                  "keep=99999999999,discard=8", "discard"])
def test_parse_refuses_and_leaves_the_outputs(text):
    assert _parse(text) == (ERR_ARG, -7, -9)


def test_parse_null_pointers():
    from llama_cu_awq_amd import api
    L = api.lib()
    x = C.c_int()
    assert L.q4_parse_context_shift(None, C.byref(x), C.byref(x)) == ERR_ARG
    assert L.q4_parse_context_shift(b"discard=8", None, C.byref(x)) == ERR_ARG
    assert L.q4_parse_context_shift(b"discard=8", C.byref(x), None) == ERR_ARG


def test_model_level_calls_refuse_a_null_transformer():
    from llama_cu_awq_amd import api
    L = api.lib()
    x = C.c_int()
    buf = np.zeros(64, dtype=np.float32)
    assert L.q4_shift_context(None, 10, 2, 3, 11) == ERR_ARG
    assert L.q4_set_context_shift(None, 4, 8) == ERR_ARG
    assert L.q4_get_context_shift(None, C.byref(x), C.byref(x)) == ERR_ARG
    assert L.q4_get_rope_row(None, 0, buf.ctypes.data) == ERR_ARG


def test_op_refuses_bad_arguments_without_a_gpu():
    """every refusal is decided on the host, in front of the launch: the pointers below are never dereferenced"""
    from llama_cu_awq_amd import api
    L = api.lib()
    P = 0x1000                      # a non-null, 16-byte aligned stand-in for a device pointer

    def call(k=P, v=P, ke=P, ve=P, fmt=api.KV_FP16, layers=2, seq=77, heads=2, hs=64, n_pos=77, keep=4, D=1, cs=P):
        return L.q4_kv_shift(k, v, ke, ve, fmt, layers, seq, heads, hs, n_pos, keep, D, cs)
    assert call(k=None) == ERR_ARG and call(v=None) == ERR_ARG and call(cs=None) == ERR_ARG
    assert call(fmt=2) == ERR_ARG and call(fmt=-1) == ERR_ARG
    assert call(fmt=api.KV_FP8, ke=None) == ERR_ARG and call(fmt=api.KV_FP8, ve=None) == ERR_ARG
    for name in ("layers", "seq", "heads", "hs", "n_pos", "D"):
        assert call(**{name: 0}) == ERR_ARG, name
        assert call(**{name: -1}) == ERR_ARG, name
    assert call(keep=-1) == ERR_ARG
    assert call(hs=33) == ERR_ARG                                   # odd
    for hs in (32, 96, 80, 512):
        assert call(fmt=api.KV_FP8, hs=hs) == ERR_ARG               # the FP8 format's head sizes are 64, 128, 256
    assert call(fmt=api.KV_FP8, k=P + 8) == ERR_ARG                 # an FP8 base off the 16-byte grid
    assert call(n_pos=78) == ERR_ARG                                # above seq_len
    assert call(n_pos=10, keep=4, D=7) == ERR_ARG                   # keep + D > n_pos
    assert call(n_pos=10, keep=2 ** 31 - 1, D=2 ** 31 - 1) == ERR_ARG


# ---- the restatement against the oracle's RoPE --------------------------------------------------------------------------------------------------------
CASES = [(32, 1e4, 5, 1), (32, 1e6, 64, 63), (64, 1e4, 320, 100), (64, 1e6, 1300, 650), (80, 1e4, 300, 149), (96, 1e4, 2047, 1022), (128, 1e4, 2048, 1),
         (128, 1e6, 16000, 8000), (256, 1e4, 16000, 8000), (256, 1e6, 600, 298), (128, 1e4, 16383, 8190)]


@pytest.mark.parametrize("head_size, theta, p, D", CASES)
def test_restatement_agrees_with_the_oracles_rope(orc, head_size, theta, p, D):
    """shift(rope(k, p), D) against rope(k, p - D), every element within 3 * 2^-11 * hypot(pair) + 3 * 2^-25 (context_shift_ref.tolerance: derived from
    the three roundings to half, not measured; a numpy dry run of exactly this reached 0.67 of it)."""
    rng = np.random.default_rng(head_size * 1000 + p)
    heads, hp = 4, head_size // 2
    table = ref.rope_table_row(D, head_size, theta)
    worst = 0.0
    for scale in (1e-6, 1e-3, 1.0, 30.0, 3000.0):
        k = (rng.standard_normal(heads * head_size) * scale).astype(np.float16)
        k[:4] = [0.0, -0.0, 6e-8, -6e-8]                         # zeros and subnormals among the rest
        q = np.zeros_like(k)
        stored = orc.rope(q, k, heads, heads, head_size, p, theta)[1]
        direct = orc.rope(q, k, heads, heads, head_size, p - D, theta)[1]
        got = ref.rotate(stored, head_size, table)
        d64 = direct.astype(np.float64).reshape(heads, head_size)
        hyp = np.hypot(d64[:, :hp], d64[:, hp:])
        tol = ref.tolerance(np.concatenate([hyp, hyp], axis=1))
        err = np.abs(got.astype(np.float64).reshape(heads, head_size) - d64)
        assert np.isfinite(err).all()
        worst = max(worst, float((err / tol).max()))
        assert (err <= tol).all(), "scale %g: %g of the bound" % (scale, (err / tol).max())
    print("head_size %d theta %g (p, D) = (%d, %d): worst %.3f of the bound" % (head_size, theta, p, D, worst))


def test_restatement_moves_rows_and_leaves_the_rest():
    rng = np.random.default_rng(5)
    k = rng.standard_normal((2, 20, 64)).astype(np.float16)
    v = rng.standard_normal((2, 20, 64)).astype(np.float16)
    k0, v0 = k.copy(), v.copy()
    table = ref.rope_table_row(5, 32, 1e4)
    ref.shift_fp16(k, v, 17, 3, 5, 32, table)
    assert np.array_equal(v[:, 3:12], v0[:, 8:17]) and np.array_equal(v[:, :3], v0[:, :3]) and np.array_equal(v[:, 12:], v0[:, 12:])
    assert np.array_equal(k[:, 3:12], ref.rotate(k0[:, 8:17], 32, table)) and np.array_equal(k[:, :3], k0[:, :3]) and np.array_equal(k[:, 12:], k0[:, 12:])
    ident = np.stack([np.ones(16, np.float32), np.zeros(16, np.float32)], axis=1)
    assert np.array_equal(ref.rotate(k0, 32, ident).view(np.uint16), k0.view(np.uint16))       # D = 0's table is the identity, bit for bit
