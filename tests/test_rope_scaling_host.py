"""RoPE scaling without a GPU: the new symbols, the setter's and the parser's refusals, q4_rope_inv_freq against the numpy float64 restatement
(rope_scaling_ref), and the restatement's rotation against the oracle's own RoPE."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import rope_scaling_ref as ref
from conftest import ROOT, assert_close_f16

ERR_ARG = 5
NEW = ["q4_set_rope_scaling", "q4_get_rope_scaling", "q4_rope_scaling_of", "q4_parse_rope_scaling", "q4_rope_inv_freq", "q4_get_rope_inv_freq",
       "q4_rope_rotation_freqs"]
LLAMA3 = {"rope_type": "llama3", "factor": 8.0, "low_freq_factor": 1.0, "high_freq_factor": 4.0}
# (head_size, theta, original_max_position_embeddings): all three Llama-3 bands are populated; the last is Llama-3.1's own
BAND_CASES = [(32, 1e4, 64, (2, 3, 11)), (16, 1e4, 64, (1, 2, 5)), (128, 5e5, 8192, (29, 6, 29))]


def _api():
    from llama_cu_awq_amd import api
    return api


def test_every_new_symbol_is_declared_exported_and_listed():
    api = _api()
    header = open(os.path.join(ROOT, "include", "llama2_q4.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    exports = open(os.path.join(ROOT, "llama_cu_awq_amd", "csrc", "exports.map")).read()
    assert "q4_*" in exports                                    # the version script lets every q4_ symbol out
    out = subprocess.check_output(["nm", "-D", "--defined-only", api.LIB_PATH]).decode()
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in exported, name
        assert name in api.SYMBOLS, name
        assert getattr(api.lib(), name).argtypes is not None, name
    for name in ("Q4_ROPE_NONE = 0", "Q4_ROPE_LINEAR = 1", "Q4_ROPE_LLAMA3 = 2", "Q4_ROPE_CUSTOM = 3", "Q4_ROPE_MAX_PAIRS = 256"):
        assert name in header, name
    assert (api.ROPE_NONE, api.ROPE_LINEAR, api.ROPE_LLAMA3, api.ROPE_CUSTOM, api.ROPE_MAX_PAIRS) == (0, 1, 2, 3, 256)


def _get():
    api = _api()
    r = api.RopeScaling()
    assert api.lib().q4_get_rope_scaling(C.byref(r)) == 0
    return r


def _fields(r):
    return (r.kind, r.factor, r.low_freq_factor, r.high_freq_factor, r.original_max_position, r.n_freqs)


@pytest.fixture()
def setting():
    """the process-wide setting starts and ends at NONE"""
    api = _api()
    assert api.lib().q4_set_rope_scaling(None) == 0
    yield api
    assert api.lib().q4_set_rope_scaling(None) == 0


def test_setter_round_trips(setting):
    api, L = setting, setting.lib()
    assert _get().kind == api.ROPE_NONE and not _get().inv_freq
    assert L.q4_set_rope_scaling(C.byref(api.RopeScaling(kind=api.ROPE_LINEAR, factor=4.0))) == 0
    assert _fields(_get()) == (api.ROPE_LINEAR, 4.0, 0.0, 0.0, 0, 0)
    r = api.RopeScaling(kind=api.ROPE_LLAMA3, factor=8.0, low_freq_factor=1.0, high_freq_factor=4.0, original_max_position=8192)
    assert L.q4_set_rope_scaling(C.byref(r)) == 0
    assert _fields(_get()) == (api.ROPE_LLAMA3, 8.0, 1.0, 4.0, 8192, 0)
    freqs = np.linspace(1.0, 0.0, 16, dtype=np.float32)
    r, keep = api.rope_scaling_struct({"kind": "custom", "inv_freq": freqs.copy()})
    assert L.q4_set_rope_scaling(C.byref(r)) == 0
    keep[:] = -1.0                                              # the library holds a copy
    got = _get()
    assert got.kind == api.ROPE_CUSTOM and got.n_freqs == 16 and np.array_equal(np.array(got.inv_freq[:16], dtype=np.float32), freqs)
    assert L.q4_set_rope_scaling(C.byref(api.RopeScaling(kind=api.ROPE_NONE, factor=-3.0))) == 0       # NONE: off, its other fields are not read
    assert _fields(_get()) == (api.ROPE_NONE, 0.0, 0.0, 0.0, 0, 0)
    assert L.q4_get_rope_scaling(None) == ERR_ARG


def _bad_settings(api):
    inf, nan = float("inf"), float("nan")
    lin = lambda f: api.RopeScaling(kind=api.ROPE_LINEAR, factor=f)
    l3 = lambda f=8.0, lo=1.0, hi=4.0, orig=8192: api.RopeScaling(kind=api.ROPE_LLAMA3, factor=f, low_freq_factor=lo, high_freq_factor=hi,
                                                                   original_max_position=orig)
    out = [("kind 4", api.RopeScaling(kind=4, factor=2.0)), ("kind -1", api.RopeScaling(kind=-1, factor=2.0))]
    out += [("linear factor %r" % f, lin(f)) for f in (0.5, 0.0, -2.0, inf, nan, 0.99999994)]
    out += [("llama3 factor %r" % f, l3(f=f)) for f in (0.5, inf, nan)]
    out += [("llama3 low %r" % lo, l3(lo=lo)) for lo in (0.0, -1.0, nan, inf, 4.0, 5.0)]
    out += [("llama3 high %r" % hi, l3(hi=hi)) for hi in (1.0, 0.5, nan, inf)]
    out += [("llama3 orig %r" % o, l3(orig=o)) for o in (0, -8192)]
    good = np.ones(8, dtype=np.float32)
    ptr = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    out += [("custom n_freqs %d" % n, api.RopeScaling(kind=api.ROPE_CUSTOM, n_freqs=n, inv_freq=ptr(np.ones(300, dtype=np.float32)))) for n in (0, -1, 257)]
    out += [("custom null", api.RopeScaling(kind=api.ROPE_CUSTOM, n_freqs=8))]
    for v in (-1e-3, inf, -inf, nan):
        a = good.copy()
        a[5] = v
        out.append(("custom entry %r" % v, api.RopeScaling(kind=api.ROPE_CUSTOM, n_freqs=8, inv_freq=ptr(a)), a))
    return out


def test_setter_refuses_and_leaves_the_setting(setting):
    api, L = setting, setting.lib()
    assert L.q4_set_rope_scaling(C.byref(api.RopeScaling(kind=api.ROPE_LINEAR, factor=4.0))) == 0
    cases = _bad_settings(api)
    assert len(cases) >= 30
    out = np.zeros(4, dtype=np.float32)
    for case in cases:
        assert L.q4_set_rope_scaling(C.byref(case[1])) == ERR_ARG, case[0]
        assert _fields(_get()) == (api.ROPE_LINEAR, 4.0, 0.0, 0.0, 0, 0), case[0]
        assert L.q4_rope_inv_freq(C.byref(case[1]), 8, 1e4, out.ctypes.data) == ERR_ARG, case[0]       # the host computation checks the same way


def _parse(text):
    api = _api()
    r = api.RopeScaling(kind=-7, factor=-9.0, n_freqs=-5)
    rc = api.lib().q4_parse_rope_scaling(text.encode(), C.byref(r))
    return rc, _fields(r)


def test_parse_round_trips(setting):
    api, L = setting, setting.lib()
    assert _parse("none") == (0, (0, 0.0, 0.0, 0.0, 0, 0))
    assert _parse("linear,factor=4") == (0, (1, 4.0, 0.0, 0.0, 0, 0))
    assert _parse("linear,factor=1") == (0, (1, 1.0, 0.0, 0.0, 0, 0))
    assert _parse("linear,factor=2.5") == (0, (1, 2.5, 0.0, 0.0, 0, 0))
    assert _parse("llama3,factor=8,low=1,high=4,orig=8192") == (0, (2, 8.0, 1.0, 4.0, 8192, 0))
    assert _parse("llama3,orig=64,high=4.5,factor=32,low=.5") == (0, (2, 32.0, 0.5, 4.5, 64, 0))
    # text -> struct -> setting -> struct, and the Python forms land on the same struct
    for text, hf in (("linear,factor=4", {"type": "linear", "factor": 4.0}),
                     ("llama3,factor=8,low=1,high=4,orig=8192", dict(LLAMA3, original_max_position_embeddings=8192))):
        r = api.RopeScaling()
        assert L.q4_parse_rope_scaling(text.encode(), C.byref(r)) == 0 and L.q4_set_rope_scaling(C.byref(r)) == 0
        assert _fields(_get()) == _fields(r) == _fields(api.rope_scaling_struct(hf)[0]) == _fields(api.rope_scaling_struct(text)[0])
        assert _get().as_dict() == {("rope_type" if k == "type" else k): v for k, v in hf.items()}


@pytest.mark.parametrize("text", ["", "None", "yarn,factor=4", "linear", "linear,", "linear,factor=", "linear,factor=0.5", "linear,factor=x", "linear,factor=4x",
                                  "linear,factor=-4", "linear,factor=+4", "linear,factor= 4", "linear,factor=inf", "linear,factor=nan", "linear,factor=1e99",
                                  "linear,factor=4,factor=4", "linear,factor=4,low=1", "linear,factor=4,", "linear,=4", "linear,factor", "none,factor=2",
                                  "none,", ",linear,factor=4", "factor=4", "llama3", "llama3,factor=8", "llama3,factor=8,low=1,high=4",
                                  "llama3,factor=8,low=4,high=4,orig=8192", "llama3,factor=8,low=0,high=4,orig=8192", "llama3,factor=8,low=1,high=4,orig=0",
                                  "llama3,factor=8,low=1,high=4,orig=8192.5", "llama3,factor=8,low=1,high=4,orig=99999999999",
                                  "llama3,factor=8,low=1,high=4,orig=8192,extra=1", "llama3,factor=8,low=1,high=4,orig=-1", "custom,n_freqs=4", "linearx,factor=4"])
def test_parse_refuses_and_leaves_the_output(text):
    assert _parse(text) == (ERR_ARG, (-7, -9.0, 0.0, 0.0, 0, -5))


def test_null_pointers_and_model_level_calls_without_a_model():
    api = _api()
    L = api.lib()
    r = api.RopeScaling()
    out = np.zeros(64, dtype=np.float32)
    assert L.q4_parse_rope_scaling(None, C.byref(r)) == ERR_ARG and L.q4_parse_rope_scaling(b"none", None) == ERR_ARG
    assert L.q4_rope_scaling_of(None, C.byref(r)) == ERR_ARG
    assert L.q4_get_rope_inv_freq(None, out.ctypes.data) == ERR_ARG
    assert L.q4_rope_inv_freq(None, 32, 1e4, None) == ERR_ARG
    for head_size in (0, -2, 1, 33):
        assert L.q4_rope_inv_freq(None, head_size, 1e4, out.ctypes.data) == ERR_ARG, head_size
    for theta in (0.0, -1e4, float("inf"), float("nan")):
        assert L.q4_rope_inv_freq(None, 32, theta, out.ctypes.data) == ERR_ARG, theta
    custom, keep = api.rope_scaling_struct({"kind": "custom", "inv_freq": np.ones(8, dtype=np.float32)})
    assert L.q4_rope_inv_freq(C.byref(custom), 32, 1e4, out.ctypes.data) == ERR_ARG        # 8 frequencies for 16 pairs
    P = 0x1000                                                                              # a stand-in device pointer: refused before any launch
    assert L.q4_rope_rotation_freqs(P, P, 4, 4, 33, P, 0, P) != 0 and L.q4_rope_rotation_freqs(P, P, 4, 4, 64, P, 0, None) == ERR_ARG
    assert L.q4_rope_rotation_freqs(P, P, 4, 5, 64, P, 0, P) == ERR_ARG and L.q4_rope_rotation_freqs(None, P, 4, 4, 64, P, 0, P) == ERR_ARG


# ---- the frequencies against the restatement -----------------------------------------------------------------------------------------------------------
def _scalings():
    out = [None] + [{"type": "linear", "factor": f} for f in (1.0, 2.0, 4.0, 8.0, 3.0, 1.5)]
    out += [dict(LLAMA3, original_max_position_embeddings=o) for o in (64, 8192, 2 ** 30)]
    out += [{"rope_type": "llama3", "factor": 32.0, "low_freq_factor": 1.0, "high_freq_factor": 4.0, "original_max_position_embeddings": 8192},   # Llama-3.2
            {"rope_type": "llama3", "factor": 3.0, "low_freq_factor": 0.75, "high_freq_factor": 5.5, "original_max_position_embeddings": 300}]
    return out


@pytest.mark.parametrize("head_size, theta", [(32, 1e4), (16, 1e4), (128, 5e5), (64, 1e4), (128, 1e6), (256, 1e4), (80, 1e4), (2, 1e4), (512, 5e5)])
def test_inv_freq_is_the_restatement_within_one_ulp(head_size, theta):
    """computed in double and rounded once: the two pow()s may differ in the last double bit, which can flip only the final rounding"""
    api = _api()
    for scaling in _scalings():
        got = api.rope_inv_freq(scaling, head_size, theta)
        want = ref.inv_freq32(scaling, head_size, theta)
        assert got.dtype == np.float32 and got.shape == (head_size // 2,)
        d = ref.ulp_diff32(got, want)
        assert d.max() <= 1, (scaling, int(d.argmax()), got[d.argmax()], want[d.argmax()])
        assert got[0] == (1.0 if scaling is None or scaling.get("type") != "linear" else np.float32(1.0 / scaling["factor"]))


@pytest.mark.parametrize("head_size, theta, orig, bands", BAND_CASES)
def test_inv_freq_is_exact_where_the_arithmetic_is(head_size, theta, orig, bands):
    api = _api()
    base = api.rope_inv_freq(None, head_size, theta)
    assert np.array_equal(api.rope_inv_freq("none", head_size, theta), base)
    assert (np.diff(base) < 0).all()
    for factor in (2.0, 4.0, 8.0):                  # a power of two: round(f / factor) == round(f) / factor
        got = api.rope_inv_freq({"type": "linear", "factor": factor}, head_size, theta)
        assert np.array_equal(got.view(np.uint32), (base / np.float32(factor)).view(np.uint32)), factor
        assert np.array_equal(got, api.rope_inv_freq("linear,factor=%g" % factor, head_size, theta))
        assert (np.diff(got) < 0).all()
    scaling = dict(LLAMA3, original_max_position_embeddings=orig)
    high, middle, low = ref.llama3_bands(scaling, head_size, theta)
    assert (len(high), len(middle), len(low)) == bands and len(high) + len(middle) + len(low) == head_size // 2
    got = api.rope_inv_freq(scaling, head_size, theta)
    assert np.array_equal(got[high].view(np.uint32), base[high].view(np.uint32))
    assert np.array_equal(got[low].view(np.uint32), (base[low] / np.float32(8.0)).view(np.uint32))
    assert ((got[middle] < base[middle]) & (got[middle] > base[middle] / np.float32(8.0))).all()
    assert (np.diff(got) < 0).all()                 # strictly decreasing through all three bands
    assert np.array_equal(got, api.rope_inv_freq("llama3,factor=8,low=1,high=4,orig=%d" % orig, head_size, theta))
    rng = np.random.default_rng(head_size)
    custom = rng.uniform(0.0, 2.0, head_size // 2).astype(np.float32)
    custom[0], custom[-1] = 0.0, np.float32(1e-45)  # zero and the smallest subnormal pass through as they are
    assert np.array_equal(api.rope_inv_freq({"kind": "custom", "inv_freq": custom}, head_size, theta).view(np.uint32), custom.view(np.uint32))


def test_python_forms():
    api = _api()
    with pytest.raises(ValueError):
        api.rope_scaling_struct({"rope_type": "yarn", "factor": 4.0})
    with pytest.raises(ValueError):
        api.rope_scaling_struct("yarn,factor=4")
    with pytest.raises(ValueError):
        api.rope_scaling_struct(4.0)
    with pytest.raises(KeyError):
        api.rope_scaling_struct({"rope_type": "llama3", "factor": 8.0})
    assert api.rope_scaling_struct(None)[0].kind == api.ROPE_NONE and api.rope_scaling_struct({"rope_type": "default"})[0].kind == api.ROPE_NONE
    with pytest.raises(api.Q4Error):
        api.rope_inv_freq({"type": "linear", "factor": 0.5}, 32, 1e4)


# ---- the restatement's rotation against the oracle's RoPE ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("heads,kv_heads,hs,pos,theta", [(32, 32, 128, 0, 1e4), (32, 32, 128, 255, 1e4), (8, 2, 64, 17, 1e4), (4, 4, 64, 2047, 1e4),
                                                         (32, 32, 128, 255, 5e5), (8, 2, 64, 17, 5e5)])
def test_restatement_rotation_agrees_with_the_oracles_rope(orc, rng, heads, kv_heads, hs, pos, theta):
    """given the base frequencies of theta the restated rotation is the oracle's, under the arguments test_ops_gpu.py::test_rope holds the device's to (its
    four cases, theta 1e4): this pins the pairing (i, i + head_size/2) and the signs before any scaled kernel runs. The oracle's frequency is 1 / powf in
    fp32, the restatement's the float64 power rounded once: up to an ulp or two apart, an angle difference of pos * 2^-23 rad at most -- so the cases at
    Llama-3's theta 5e5 stay at positions where that is far below half an fp16 ulp of the outputs (255: 3e-5)."""
    q = rng.standard_normal(heads * hs).astype(np.float16)
    k = rng.standard_normal(kv_heads * hs).astype(np.float16)
    rq, rk = orc.rope(q, k, heads, kv_heads, hs, pos, theta)
    gq, gk = ref.rotate(q, k, heads, kv_heads, hs, pos, ref.inv_freq32(None, hs, theta))
    assert_close_f16(gq, rq, max_frac=0.05, what="rope q")
    assert_close_f16(gk, rk, max_frac=0.05, what="rope k")
