"""Sampling controls without a GPU: the numpy reference (tests/sampling_controls_ref.py) on hand-made cases, the text parser, and every argument
check of the setters and of the op-level launcher -- none of which may touch the GPU."""
import ctypes as C

import numpy as np
import pytest

import sampling_controls_ref as ref

ERR_ARG = 5
F = np.float32


def _h(*v):
    return np.array(v, dtype=np.float16)


# ---------------------------------------------------------------------------------------------------------------------------------
# the reference
def test_order_of_the_operations():
    """bias first, then the repetition penalty on the BIASED value, then frequency / presence, one rounding to half at the end"""
    x = _h(1.0, 2.0, -1.0, 0.5)
    got = ref.process(x, repeat_penalty=2.0, presence_penalty=0.5, frequency_penalty=0.25, penalty_last_n=8, logit_bias={1: -3.0, 3: 1.0},
                      tokens=[1, 1, 2], pos=2)
    # token 1: (2 - 3) = -1 -> negative: * 2 = -2 -> - (2 * 0.25 + 0.5) = -3;  token 2: -1 * 2 - (0.25 + 0.5) = -2.75;  token 3: bias only
    assert got.tolist() == [1.0, -3.0, -2.75, 1.5]
    # a case the other order (penalty, then bias) gets wrong: (-1 + 3) / 4 = 0.5, not -1 * 4 + 3 = -1
    got = ref.process(_h(-1.0), repeat_penalty=4.0, penalty_last_n=4, logit_bias={0: 3.0}, tokens=[0], pos=0)
    assert got.tolist() == [0.5]
    # one rounding: 0.1 (half: 0.0999755859375) / 3 in float32, rounded to half once
    got = ref.process(_h(0.1), repeat_penalty=3.0, penalty_last_n=1, tokens=[0], pos=0)
    assert got[0] == np.float16(F(np.float16(0.1)) / F(3.0))


def test_positive_and_negative_logits_under_the_repetition_penalty_and_counts():
    x = _h(3.0, -3.0, 0.0, 5.0)
    got = ref.process(x, repeat_penalty=1.5, penalty_last_n=64, tokens=[0, 1, 2, 0, 0], pos=4)
    assert got.tolist() == [2.0, -4.5, 0.0, 5.0]               # v > 0: divided; v <= 0: multiplied; untouched entries keep their bits
    got = ref.process(x, frequency_penalty=0.5, presence_penalty=1.0, tokens=[0, 1, 0, 0, 9, -4, 4], pos=6)
    assert got.tolist() == [3.0 - (3 * 0.5 + 1.0), -3.0 - (0.5 + 1.0), 0.0, 5.0]      # counts above 1; ids outside [0, n) are ignored
    # the window: the last penalty_last_n entries up to and including pos, never what lies behind pos
    got = ref.process(x, presence_penalty=1.0, penalty_last_n=2, tokens=[0, 1, 2, 3], pos=2)
    assert got.tolist() == [3.0, -4.0, -1.0, 5.0]
    assert ref.window([5, 6, 7, 8], 1, 64).tolist() == [5, 6] and ref.window([5, 6, 7, 8], 3, 0).size == 0
    # neutral penalties read no window at all
    assert ref.process(x, penalty_last_n=64, tokens=[0, 1], pos=1).tobytes() == x.tobytes()


def test_top_k_ties_and_special_values():
    x = _h(1.0, 3.0, 3.0, -np.inf, 3.0, -0.0, 0.0, np.nan, 1.0)
    got = ref.process(x, top_k=2)
    assert np.array_equal(np.isneginf(got), [True, False, False, True, True, True, True, True, True])      # the tie at rank 2: lowest indices stay
    got = ref.process(x, top_k=5)                                                                           # 3, 3, 3, then 1 (index 0), 1 (index 8)
    assert np.array_equal(np.isneginf(got), [False, False, False, True, False, True, True, True, False])
    got = ref.process(x, top_k=6)                                                                           # -0 at index 5 ties with +0 at 6: index decides
    assert not np.isneginf(got[5]) and np.isneginf(got[6]) and got[5:6].view(np.uint16)[0] == 0x8000       # ... and keeps its sign bit
    got = ref.process(x, top_k=8)                                                                           # the NaN ranks last, behind -inf
    assert np.isneginf(got[7]) and np.isneginf(got[3])
    got = ref.process(x, top_k=9)
    assert got.tobytes() == x.tobytes()                        # k = n: nothing changes, the NaN keeps its bits
    assert ref.half_key(_h(-0.0))[0] == ref.half_key(_h(0.0))[0] and ref.half_key(_h(np.nan))[0] == 0 < ref.half_key(_h(-np.inf))[0]


def test_clamp_infinities_and_nan():
    x = _h(60000.0, -60000.0, -np.inf, np.inf, 1.0)
    got = ref.process(x, logit_bias={0: 60000.0, 1: -60000.0, 2: 5.0, 3: -np.inf, 4: -np.inf})
    assert got[0] == np.float16(65504.0) and got[1] == np.float16(-65504.0)          # finite: clamped, not +-inf
    assert np.isneginf(got[2])                                                       # -inf stays -inf
    assert got[3:4].view(np.uint16)[0] == 0x7E00                                     # inf - inf: the quiet NaN
    assert np.isneginf(got[4])                                                       # a ban
    got = ref.process(_h(np.nan, 2.0), presence_penalty=1.0, tokens=[0, 1], pos=1)
    assert got.view(np.uint16)[0] == 0x7E00 and got[1] == 1.0


def test_min_p_is_on_the_processed_logits():
    x = _h(4.0, 3.0, 1.0, 0.0, -np.inf)
    thr = float(np.log(0.1))                                                         # -2.30
    got = ref.process(x, min_p=0.1)
    assert np.array_equal(np.isneginf(got), [False, False, True, True, True]) and thr < -2
    got = ref.process(x, min_p=0.1, logit_bias={0: -np.inf})                         # the maximum is banned first: m = 3
    assert np.array_equal(np.isneginf(got), [True, False, False, True, True])
    got = ref.process(x, min_p=0.1, top_k=1)
    assert np.array_equal(np.isneginf(got), [False, True, True, True, True])
    assert ref.min_p_margin(x, 0.1) > 0.1


# ---------------------------------------------------------------------------------------------------------------------------------
# the parser
def test_parser_round_trip_and_errors():
    from llama_cu_awq_amd import api
    L = api.lib()
    c = api.parse_sampling_controls("top_k=40,min_p=0.05,repeat_penalty=1.1,last_n=64,presence=0,frequency=0")
    assert c.as_dict() == dict(top_k=40, min_p=F(0.05), repeat_penalty=F(1.1), presence_penalty=0.0, frequency_penalty=0.0, penalty_last_n=64)
    c = api.parse_sampling_controls("frequency=0.25,last_n=1024,presence=-0.5")      # any subset, any order; the rest neutral
    assert c.as_dict() == dict(top_k=0, min_p=0.0, repeat_penalty=1.0, presence_penalty=-0.5, frequency_penalty=0.25, penalty_last_n=1024)
    text = "top_k=%d,min_p=%r,repeat_penalty=%r,last_n=%d,presence=%r,frequency=%r" % (
        7, float(F(0.3)), float(F(1.3)), 16, float(F(0.5)), float(F(0.25)))
    c = api.parse_sampling_controls(text)
    assert c.as_dict() == dict(top_k=7, min_p=F(0.3), repeat_penalty=F(1.3), presence_penalty=0.5, frequency_penalty=0.25, penalty_last_n=16)
    assert api.parse_sampling_controls("").as_dict() == api.SamplingControls().as_dict()
    out = api.SamplingControls(top_k=3)
    for bad in ("top_p=0.9", "top_k", "top_k=", "=4", "top_k=4x", "min_p=abc", "top_k=1.5", "top_k=4,", ",top_k=4", "top_k=4,,min_p=0.1", "top_k=-1",
                "min_p=1", "repeat_penalty=0", "last_n=1025", "presence=nan", "frequency=inf", "min_p=0.1 "):
        assert L.q4_parse_sampling_controls(bad.encode(), C.byref(out)) == ERR_ARG, bad
        assert out.top_k == 3, "a failed parse wrote its output"
    assert L.q4_parse_sampling_controls(None, C.byref(out)) == ERR_ARG and L.q4_parse_sampling_controls(b"top_k=1", None) == ERR_ARG


# ---------------------------------------------------------------------------------------------------------------------------------
# the argument checks
@pytest.fixture()
def sampler():
    """a Sampler the test builds itself: the struct of include/llama2_q4.h, zeroed (no device buffer: nothing here may touch the GPU)"""
    from llama_cu_awq_amd import api
    L = api.lib()
    L.destroy_sampler.argtypes = [C.c_void_p]
    L.destroy_sampler.restype = None
    buf = C.create_string_buffer(64)
    yield C.cast(buf, C.c_void_p)
    L.destroy_sampler(C.cast(buf, C.c_void_p))                  # forgets the controls kept beside it


def test_setter_argument_checks(sampler):
    from llama_cu_awq_amd import api
    L = api.lib()
    SC = api.SamplingControls
    good = SC(top_k=40, min_p=0.05, repeat_penalty=1.1, presence_penalty=0.5, frequency_penalty=-0.25, penalty_last_n=1024)
    got = SC()
    assert L.q4_sampler_get_controls(sampler, C.byref(got)) == 0 and got.as_dict() == SC(penalty_last_n=0).as_dict()      # never set: neutral
    assert L.q4_sampler_set_controls(sampler, C.byref(good)) == 0
    assert L.q4_sampler_get_controls(sampler, C.byref(got)) == 0 and got.as_dict() == good.as_dict()
    nan, inf = float("nan"), float("inf")
    for kw in (dict(top_k=-1), dict(min_p=-0.1), dict(min_p=1.0), dict(min_p=nan), dict(repeat_penalty=0.0), dict(repeat_penalty=-1.0),
               dict(repeat_penalty=inf), dict(repeat_penalty=nan), dict(presence_penalty=inf), dict(presence_penalty=nan),
               dict(frequency_penalty=-inf), dict(frequency_penalty=nan), dict(penalty_last_n=-1), dict(penalty_last_n=1025)):
        assert L.q4_sampler_set_controls(sampler, C.byref(SC(**kw))) == ERR_ARG, kw
        assert L.q4_sampler_get_controls(sampler, C.byref(got)) == 0 and got.as_dict() == good.as_dict(), "a refused call changed the controls"
    assert L.q4_sampler_set_controls(None, C.byref(good)) == ERR_ARG
    assert L.q4_sampler_get_controls(None, C.byref(got)) == ERR_ARG and L.q4_sampler_get_controls(sampler, None) == ERR_ARG
    assert L.q4_sampler_set_controls(sampler, C.byref(SC(penalty_last_n=0))) == 0 and L.q4_sampler_set_controls(sampler, None) == 0   # neutral, NULL: off

    def bias(ids, vals):
        a, b = np.array(ids, dtype=np.int32), np.array(vals, dtype=np.float32)
        return L.q4_sampler_set_logit_bias(sampler, a.ctypes.data, b.ctypes.data, len(ids))
    assert bias([5, 7, 9], [1.0, -inf, -65504.0]) == 0          # -inf: a ban
    assert bias(list(range(256)), [0.5] * 256) == 0
    assert bias(list(range(257)), [0.5] * 257) == ERR_ARG
    assert bias([5, 7, 5], [1.0, 2.0, 3.0]) == ERR_ARG          # listed twice
    assert bias([5, -1], [1.0, 2.0]) == ERR_ARG
    assert bias([5], [nan]) == ERR_ARG and bias([5], [inf]) == ERR_ARG and bias([5], [65536.0]) == ERR_ARG and bias([5], [-70000.0]) == ERR_ARG
    assert L.q4_sampler_set_logit_bias(sampler, None, None, 2) == ERR_ARG and L.q4_sampler_set_logit_bias(sampler, None, None, -1) == ERR_ARG
    assert L.q4_sampler_set_logit_bias(None, None, None, 0) == ERR_ARG
    assert bias([], []) == 0                                    # n = 0 clears


def test_op_level_argument_checks_touch_no_gpu():
    """every pointer here is a host pointer or a made-up address: a call that got as far as the GPU would fail otherwise than with Q4_ERR_ARG"""
    from llama_cu_awq_amd import api
    L = api.lib()
    SC = api.SamplingControls
    fake = C.c_void_p(0x1000)
    ids, vals = np.array([1, 2], dtype=np.int32), np.array([1.0, 2.0], dtype=np.float32)
    call = lambda logits, n, c, i=None, b=None, nb=0: L.q4_process_logits(logits, n, C.byref(c) if c is not None else None, i, b, nb, None, None)
    assert call(None, 8, SC(top_k=2)) == ERR_ARG
    assert call(fake, 0, SC(top_k=2)) == ERR_ARG
    assert call(fake, 8, None) == ERR_ARG
    assert call(fake, 8, SC(top_k=9)) == ERR_ARG                # top_k > n
    assert call(fake, 8, SC(top_k=-1)) == ERR_ARG and call(fake, 8, SC(min_p=1.5)) == ERR_ARG and call(fake, 8, SC(repeat_penalty=0.0)) == ERR_ARG
    assert call(fake, 2, SC(), ids.ctypes.data, vals.ctypes.data, 2) == ERR_ARG      # id 2 >= n
    assert call(fake, 8, SC(), ids.ctypes.data, None, 2) == ERR_ARG and call(fake, 8, SC(), None, None, 257) == ERR_ARG
    assert call(fake, 8, SC()) == 0                             # all neutral, no bias: nothing to launch


def test_python_front_end_builds_the_arrays():
    from llama_cu_awq_amd import api
    ids, bias = api._bias_arrays({7: -1.5, 3: float("-inf")})
    assert ids.tolist() == [3, 7] and ids.dtype == np.int32 and bias.dtype == np.float32 and np.isneginf(bias[0]) and bias[1] == -1.5
    assert api._bias_arrays(None)[0].shape == (0,)
    assert api.SamplingControls().as_dict() == dict(ref.NEUTRAL)
    assert {"q4_sampler_set_controls", "q4_sampler_get_controls", "q4_sampler_set_logit_bias", "q4_parse_sampling_controls",
            "q4_process_logits"} <= set(api.SYMBOLS)
