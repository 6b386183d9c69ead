"""The FP8 K / V cache format on the CPU: the numpy quantiser's round trip is exact in fp16, the composed forward that the GPU tests
compare against equals the oracle's own forward bit for bit when its round trip is off, and the library's format setting loads,
round-trips and rejects bad values without a GPU."""
import numpy as np
import pytest

import kv8_ref
from llama_cu_awq_amd import synth

HS = 64


def _rows(kind, rng):
    x = rng.standard_normal((48, 4 * HS)).astype(np.float32)
    if kind == "small":
        x *= 1e-3
    elif kind == "subnormal":
        x = rng.integers(-1023, 1024, size=x.shape).astype(np.float32) * np.float32(2.0 ** -24)    # every fp16 subnormal step
    elif kind == "outlier":
        for r in range(x.shape[0]):
            for h in range(4):
                x[r, h * HS + int(rng.integers(HS))] = 300.0 if (r + h) & 1 else -300.0
    elif kind == "zero":
        x[::2] = 0.0
        x[1::2, HS: 2 * HS] = 0.0
    return x.astype(np.float16)


@pytest.mark.parametrize("kind", ["normal", "small", "subnormal", "outlier", "zero"])
def test_round_trip_is_exact_in_fp16(kind):
    x = _rows(kind, np.random.default_rng(5))
    b, e = kv8_ref.quantise(x, HS)
    assert b.dtype == np.uint8 and e.dtype == np.int8 and e.shape == (48, 4)
    assert e.min() >= kv8_ref.E_MIN and e.max() <= kv8_ref.E_MAX
    exact = kv8_ref.dequantise_f64(b, e, HS)
    rt = kv8_ref.dequantise(b, e, HS)
    assert np.array_equal(rt.astype(np.float64), exact)                      # byte * 2^e is an fp16 number
    assert not (b & 0x7F == 0x7F).any()                                      # never the NaN byte
    amax = np.abs(x.astype(np.float64)).reshape(48, 4, HS).max(axis=2)
    assert (amax <= 448.0 * 2.0 ** e.astype(np.float64)).all()               # nothing clamps below amax 57344
    smaller = e > kv8_ref.E_MIN
    assert (amax[smaller] > 448.0 * 2.0 ** (e[smaller].astype(np.float64) - 1)).all()      # ... and e is the smallest such exponent
    zero_rows = amax == 0
    assert (e[zero_rows] == kv8_ref.E_MIN).all() and (b.reshape(48, 4, HS)[zero_rows] == 0).all()
    # e4m3 keeps 4 significant bits: the round trip is within 2^-4 relative of a normal element, or half a subnormal step of the row's scale
    step = 2.0 ** (e.astype(np.float64) - 9)
    err = np.abs(rt.astype(np.float64) - x.astype(np.float64)).reshape(48, 4, HS)
    assert (err <= np.maximum(np.abs(x.astype(np.float64)).reshape(48, 4, HS) * 2.0 ** -4, step[..., None] / 2)).all()
    assert np.array_equal(kv8_ref.round_trip(rt, HS), rt)                    # idempotent


def test_saturating_row():
    x = np.zeros(HS, dtype=np.float16)
    x[3], x[7], x[9] = 60000.0, -65504.0, 1.0
    b, e = kv8_ref.quantise(x, HS)
    rt = kv8_ref.dequantise(b, e, HS)
    assert e[0] == 7 and rt[3] == 57344.0 and rt[7] == -57344.0              # 448 * 2^7: the stated deviation


@pytest.mark.parametrize("name", ["tiny", "tiny_gqa"])
def test_composed_forward_equals_the_oracle_bit_for_bit(orc, tmp_path, name):
    path = str(tmp_path / (name + ".bin"))
    synth.write_model(path, name, seed=7)
    m = orc.Model(path)
    f = kv8_ref.Forward(path, synth.geometry(name), round_trip=False)
    toks = [1, 17, 300, 45, 9, 211, 3, 77, 500, 12, 64, 8]
    for pos, tok in enumerate(toks):
        ref = m.forward(tok, pos)
        got = f.forward(tok, pos)
        assert np.array_equal(got.view(np.uint16), ref.view(np.uint16)), pos
    rk, rv = m.kv()
    assert np.array_equal(rk.view(np.uint16), f.kc.view(np.uint16)) and np.array_equal(rv.view(np.uint16), f.vc.view(np.uint16))
    m.close()


def test_round_trip_changes_the_forward(orc, tmp_path):
    """(the reference with the round trip on is a different function: the GPU test that tells FP8 from fp16 has something to tell)"""
    path = str(tmp_path / "tiny.bin")
    synth.write_model(path, "tiny", seed=7)
    a = kv8_ref.Forward(path, synth.geometry("tiny"), round_trip=False)
    b = kv8_ref.Forward(path, synth.geometry("tiny"), round_trip=True)
    for pos, tok in enumerate([1, 17, 300, 45]):
        la, lb = a.forward(tok, pos), b.forward(tok, pos)
    assert not np.array_equal(la, lb)
    assert np.array_equal(b.kc[0, :4], kv8_ref.round_trip(a.kc[0, :4], 64))   # layer 0's K does not depend on attention


def test_kv_format_setting_without_a_gpu():
    from llama_cu_awq_amd import api
    L = api.lib()
    assert L.q4_get_kv_format() == api.KV_FP16 == 0
    try:
        assert L.q4_set_kv_format(api.KV_FP8) == 0 and L.q4_get_kv_format() == 1
        for bad in (2, -1, 8):
            assert L.q4_set_kv_format(bad) == 5                                  # Q4_ERR_ARG
            assert L.q4_get_kv_format() == 1
    finally:
        assert L.q4_set_kv_format(api.KV_FP16) == 0
    assert L.q4_get_kv_format() == 0
    rs = api.RunState()
    assert L.q4_kv_format_of(rs) == api.KV_FP16                                  # a RunState the library did not build
    with pytest.raises(ValueError):
        api.Transformer("/nonexistent.bin", kv="int8")
    assert L.q4_get_kv_format() == 0
