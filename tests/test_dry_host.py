"""DRY and the no-repeat-n-gram ban without a GPU: the text parser, every argument check of the setters and of the op-level launcher (none of which
may touch the GPU), the host-computed penalty table, the numpy reference (tests/dry_ref.py) against its naive twin, the default breaker set."""
import ctypes as C
import os

import numpy as np
import pytest

import dry_ref as ref
from conftest import GOLDEN

ERR_ARG = 5
F = np.float32


def _table(**kw):
    from llama_cu_awq_amd import api
    return api.dry_penalty_table(**kw)


# ---------------------------------------------------------------------------------------------------------------------------------
# the parser
def test_parser_any_order_defaults_and_errors():
    from llama_cu_awq_amd import api
    L = api.lib()
    c = api.parse_dry("multiplier=0.8,base=1.75,allowed=2,last_n=1024,ngram=0")
    assert c.as_dict() == dict(multiplier=F(0.8), base=1.75, allowed_length=2, last_n=1024, no_repeat_ngram_size=0)
    c = api.parse_dry("ngram=4,last_n=64,multiplier=0.5")             # any subset, any order; the rest at its default
    assert c.as_dict() == dict(multiplier=0.5, base=1.75, allowed_length=2, last_n=64, no_repeat_ngram_size=4)
    c = api.parse_dry("allowed=5,base=4")
    assert c.as_dict() == dict(multiplier=0.0, base=4.0, allowed_length=5, last_n=1024, no_repeat_ngram_size=0)
    assert api.parse_dry("").as_dict() == api.DryControls().as_dict() == dict(ref.DEFAULT)
    out = api.DryControls(allowed_length=7)
    for bad in ("window=3", "multiplier", "multiplier=", "=4", "ngram=4x", "base=abc", "allowed=1.5", "ngram=4,", ",ngram=4", "ngram=4,,base=2",
                "multiplier=-0.1", "multiplier=nan", "multiplier=inf", "base=0.5", "base=inf", "allowed=0", "allowed=65", "last_n=-1", "last_n=4097",
                "ngram=1", "ngram=66", "ngram=-2", "base=2 "):
        assert L.q4_parse_dry(bad.encode(), C.byref(out)) == ERR_ARG, bad
        assert out.allowed_length == 7, "a failed parse wrote its output"
    assert L.q4_parse_dry(None, C.byref(out)) == ERR_ARG and L.q4_parse_dry(b"ngram=2", None) == ERR_ARG


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
    L.destroy_sampler(C.cast(buf, C.c_void_p))                  # forgets the settings kept beside it


BAD = (dict(multiplier=-0.5), dict(multiplier=float("nan")), dict(multiplier=float("inf")), dict(base=0.5), dict(base=float("nan")),
       dict(base=float("inf")), dict(allowed_length=0), dict(allowed_length=65), dict(last_n=-1), dict(last_n=4097), dict(no_repeat_ngram_size=1),
       dict(no_repeat_ngram_size=-1), dict(no_repeat_ngram_size=66))


def test_setter_argument_checks(sampler):
    from llama_cu_awq_amd import api
    L = api.lib()
    DC = api.DryControls
    got = DC(multiplier=9.0)
    assert L.q4_sampler_get_dry(sampler, C.byref(got)) == 0 and got.as_dict() == DC().as_dict()      # never set: the defaults, off
    good = DC(multiplier=0.8, base=2.5, allowed_length=3, last_n=4096, no_repeat_ngram_size=65)
    assert L.q4_sampler_set_dry(sampler, C.byref(good)) == 0
    assert L.q4_sampler_get_dry(sampler, C.byref(got)) == 0 and got.as_dict() == good.as_dict()
    for kw in BAD:
        assert L.q4_sampler_set_dry(sampler, C.byref(DC(**kw))) == ERR_ARG, kw
        assert L.q4_sampler_get_dry(sampler, C.byref(got)) == 0 and got.as_dict() == good.as_dict(), "a refused call changed the settings"
    for kw in (dict(last_n=0), dict(allowed_length=1), dict(allowed_length=64), dict(base=1.0), dict(no_repeat_ngram_size=2)):     # the limits themselves
        assert L.q4_sampler_set_dry(sampler, C.byref(DC(**kw))) == 0, kw
    assert L.q4_sampler_set_dry(None, C.byref(good)) == ERR_ARG
    assert L.q4_sampler_get_dry(None, C.byref(got)) == ERR_ARG and L.q4_sampler_get_dry(sampler, None) == ERR_ARG
    assert L.q4_sampler_set_dry(sampler, None) == 0                                                  # NULL: off, the defaults come back
    assert L.q4_sampler_get_dry(sampler, C.byref(got)) == 0 and got.as_dict() == DC().as_dict()

    def breakers(ids):
        a = np.array(ids, dtype=np.int32)
        return L.q4_sampler_set_dry_breakers(sampler, a.ctypes.data, len(ids))
    assert breakers([13, 29901, 5]) == 0
    assert breakers(list(range(0, 3000, 3))) == 0               # hundreds of ids: no fixed limit
    assert breakers([5, 7, 5]) == ERR_ARG                       # listed twice
    assert breakers([5, -1]) == ERR_ARG
    assert L.q4_sampler_set_dry_breakers(sampler, None, 2) == ERR_ARG and L.q4_sampler_set_dry_breakers(sampler, None, -1) == ERR_ARG
    assert L.q4_sampler_set_dry_breakers(None, None, 0) == ERR_ARG
    assert breakers([]) == 0 and L.q4_sampler_set_dry_breakers(sampler, None, 0) == 0      # n = 0 clears


def test_op_level_argument_checks_touch_no_gpu():
    """every pointer here is a host pointer or a made-up address: a call that got as far as the GPU would fail otherwise than with Q4_ERR_ARG"""
    from llama_cu_awq_amd import api
    L = api.lib()
    DC = api.DryControls
    fake = C.c_void_p(0x1000)
    ids = np.array([1, 8], dtype=np.int32)
    call = lambda logits, n, c, b=None, nb=0: L.q4_dry_penalty(logits, n, C.byref(c) if c is not None else None, b, nb, fake, fake)
    on = DC(multiplier=0.8)
    assert call(None, 8, on) == ERR_ARG and call(fake, 0, on) == ERR_ARG and call(fake, 8, None) == ERR_ARG
    for kw in BAD:
        assert call(fake, 8, DC(**kw)) == ERR_ARG, kw
    assert call(fake, 8, on, ids.ctypes.data, 2) == ERR_ARG     # breaker id 8 >= n
    assert call(fake, 8, on, None, 2) == ERR_ARG and call(fake, 8, on, None, -1) == ERR_ARG
    assert call(fake, 8, DC()) == 0 and call(fake, 8, DC(multiplier=0.8, last_n=0)) == 0      # off: nothing to launch
    assert L.q4_dry_penalty(fake, 8, C.byref(on), None, 0, None, None) == 0                   # no ring: no window


# ---------------------------------------------------------------------------------------------------------------------------------
# the penalty table
@pytest.mark.parametrize("multiplier,base,allowed", [(0.8, 1.75, 2), (0.8, 1.0, 1), (3.0, 4.0, 5), (0.1, 1.1, 64), (1e30, 4.0, 2), (0.0, 1.75, 2)])
def test_penalty_table(multiplier, base, allowed):
    pen = _table(multiplier=multiplier, base=base, allowed_length=allowed)
    assert pen.shape == (65,) and pen.dtype == np.float32
    assert (pen[:allowed] == 0).all()                           # zero below allowed_length
    assert np.isfinite(pen).all() and (pen <= F(3.0e38)).all()  # the clamp keeps base 4.0 finite
    assert (np.diff(pen[allowed:].astype(np.float64)) >= 0).all()      # non-decreasing above it
    if multiplier == 0:
        assert (pen == 0).all()
        return
    assert pen[allowed] == F(multiplier)
    for L in range(allowed, 65):
        exact = float(F(multiplier)) * float(F(base)) ** (L - allowed)
        if exact < 3.0e38:                                      # within 2 ulp of float64 where that is below the clamp
            assert abs(float(pen[L]) - exact) <= 2 * float(np.spacing(F(exact))), (L, pen[L], exact)
        else:
            assert pen[L] == F(3.0e38)


def test_penalty_table_refuses_what_the_setter_refuses():
    from llama_cu_awq_amd import api
    L = api.lib()
    out = np.full(65, 7.0, dtype=np.float32)
    for kw in BAD:
        assert L.q4_dry_penalty_table(C.byref(api.DryControls(**kw)), out.ctypes.data) == ERR_ARG, kw
    assert L.q4_dry_penalty_table(None, out.ctypes.data) == ERR_ARG and L.q4_dry_penalty_table(C.byref(api.DryControls()), None) == ERR_ARG
    assert (out == 7.0).all()


# ---------------------------------------------------------------------------------------------------------------------------------
# the reference
def _h(*v):
    return np.array(v, dtype=np.float16)


def test_reference_on_hand_made_cases():
    pen = _table(multiplier=1.0, base=2.0, allowed_length=2)    # 0, 0, 1, 2, 4, ...
    kw = dict(multiplier=1.0, base=2.0, allowed_length=2, last_n=64)
    x = _h(5.0, 5.0, 5.0, 5.0)
    # ring 1 2 3 1 2: the suffix "1 2" (M = 2) was followed by 3 -> 5 - pen[2]
    got, touched = ref.apply(x, [1, 2, 3, 1, 2], 4, pen, **kw)
    assert got.tolist() == [5.0, 5.0, 5.0, 4.0] and touched == [3]
    # a match of length 1 is below allowed_length: nothing
    got, touched = ref.apply(x, [0, 2, 3, 1, 2], 4, pen, **kw)
    assert got.tolist() == x.tolist() and touched == []
    # period 1: ring 2 2 2 2, candidates at 0, 1, 2 with M = 1, 2, 3, all followed by 2: M_t = 3 -> pen[3] = 2
    got, touched = ref.apply(x, [2, 2, 2, 2], 3, pen, **kw)
    assert got.tolist() == [5.0, 5.0, 3.0, 5.0] and touched == [2]
    # a breaker inside the match shortens L_t = min(M_t, R): breaker 1 at distance 1 -> R = 1 < allowed
    got, touched = ref.apply(x, [1, 2, 3, 1, 2], 4, pen, breakers=[1], **kw)
    assert touched == []
    # ... but the ban ignores breakers: N = 3 bans what would complete a repeated 3-gram
    got, touched = ref.apply(x, [1, 2, 3, 1, 2], 4, pen, breakers=[1], multiplier=0.0, last_n=64, no_repeat_ngram_size=3)
    assert np.isneginf(got[3]) and touched == [3]
    # the window: last_n = 3 sees ring[2 .. 4] only -- no earlier "1 2"
    got, touched = ref.apply(x, [1, 2, 3, 1, 2], 4, pen, multiplier=1.0, base=2.0, allowed_length=2, last_n=3)
    assert touched == []
    # the next token outside [0, n) is ignored; position 0 and off touch nothing
    assert ref.apply(x, [1, 2, 9, 1, 2], 4, pen, **kw)[1] == [] and ref.apply(x, [1, 2], 0, pen, **kw)[1] == []
    assert ref.apply(x, [2, 2, 2], 2, pen, multiplier=0.0, last_n=64)[1] == [] and ref.apply(x, [2, 2, 2], 2, pen, multiplier=1.0, last_n=0)[1] == []
    # the finish: -inf stays, NaN becomes 0x7E00, a finite result is clamped to -65504
    big = _table(multiplier=1e30, base=2.0, allowed_length=2)
    got, _ = ref.apply(_h(-np.inf, np.nan, 3.0), [0, 0, 0, 1, 1, 1, 2, 2, 2], 2, big, multiplier=1e30, base=2.0, allowed_length=2, last_n=64)
    assert np.isneginf(got[0])
    got, _ = ref.apply(_h(1.0, np.nan, 3.0), [1, 1, 1], 2, big, multiplier=1e30, base=2.0, allowed_length=2, last_n=64)
    assert got.view(np.uint16)[1] == 0x7E00
    got, _ = ref.apply(_h(1.0, 2.0, 3.0), [2, 2, 2], 2, big, multiplier=1e30, base=2.0, allowed_length=2, last_n=64)
    assert got[2] == np.float16(-65504.0)


def _random_ring(rng, case, n):
    """alphabets of 2, 3 and 50 tokens, periodic rings, ids outside [0, n)"""
    length = int(rng.integers(2, 300))
    kind = case % 5
    if kind == 0:
        ring = rng.integers(0, 2, length)
    elif kind == 1:
        ring = rng.integers(0, 3, length)
    elif kind == 2:
        ring = rng.integers(0, min(n, 50), length)
    elif kind == 3:
        period = int(rng.integers(1, 8))
        ring = np.tile(rng.integers(0, min(n, 50), period), length // period + 1)[:length]
        if case % 2:
            ring[int(rng.integers(length))] = int(rng.integers(0, min(n, 50)))       # one flaw in the period
    else:
        ring = rng.integers(0, 4, length)
        bad = rng.choice(length, size=max(1, length // 6), replace=False)
        ring[bad] = rng.choice([-5, n, n + 7, 2 ** 31 - 1, -2 ** 31], size=bad.shape[0])
    return ring.astype(np.int32)


def test_reference_equals_the_naive_reference_on_200_random_rings():
    rng = np.random.default_rng(2024)
    touched_cases = 0
    for case in range(200):
        n = int(rng.choice([4, 60, 1000]))
        ring = _random_ring(rng, case, n)
        pos = int(rng.integers(0, ring.shape[0]))
        c = dict(multiplier=float(rng.choice([0.0, 0.8, 3.0])), base=float(rng.choice([1.0, 1.75, 4.0])), allowed_length=int(rng.choice([1, 2, 5])),
                 last_n=int(rng.choice([1, 2, 7, 64, 4096])), no_repeat_ngram_size=int(rng.choice([0, 0, 2, 3, 4, 65])))
        breakers = [] if case % 3 == 0 else [int(b) for b in rng.choice(min(n, 50), size=int(rng.integers(1, 4)), replace=False)]
        pen = _table(multiplier=c["multiplier"], base=c["base"], allowed_length=c["allowed_length"])
        x = (rng.standard_normal(n) * 3.0).astype(np.float16)
        a, ta = ref.apply(x, ring, pos, pen, breakers=breakers, **c)
        b, tb = ref.apply_naive(x, ring, pos, pen, breakers=breakers, **c)
        assert ta == tb, (case, c, breakers)
        assert a.tobytes() == b.tobytes(), (case, c, breakers)
        untouched = np.setdiff1d(np.arange(n), ta)
        assert a[untouched].tobytes() == x[untouched].tobytes()
        touched_cases += bool(ta)
    assert touched_cases >= 50, touched_cases


# ---------------------------------------------------------------------------------------------------------------------------------
# the front end
def test_default_breakers_of_the_committed_tokenizer():
    from llama_cu_awq_amd import api
    tk = api.Tokenizer(os.path.join(GOLDEN, "tokenizer.bin"), 32000)
    ids = api.dry_breaker_ids(tk)
    pieces = tk.pieces()
    newline = [i for i, p in enumerate(pieces) if p in (b"\n", b"<0x0A>")]
    assert ids and newline and set(newline) <= set(ids)
    assert all(0 <= i < 32000 for i in ids) and len(set(ids)) == len(ids)
    assert any(b":" in pieces[i] for i in ids) and any(b"*" in pieces[i] for i in ids) and any(b'"' in pieces[i] for i in ids)
    assert api.dry_breaker_ids(tk, strings=("\n",)) and set(api.dry_breaker_ids(tk, strings=("\n",))) < set(ids)
    tk.close()


def test_python_front_end():
    from llama_cu_awq_amd import api
    assert api.DryControls().as_dict() == dict(ref.DEFAULT)
    assert api.MAX_DRY_WINDOW == ref.MAX_WINDOW == 4096 and api.DRY_MAX_MATCH == ref.CAP == 64
    assert api._breaker_array({7, 3}).tolist() == [3, 7] and api._breaker_array(None).shape == (0,) and api._breaker_array([5]).dtype == np.int32
    assert {"q4_sampler_set_dry", "q4_sampler_get_dry", "q4_sampler_set_dry_breakers", "q4_parse_dry", "q4_dry_penalty_table",
            "q4_dry_penalty"} <= set(api.SYMBOLS)
