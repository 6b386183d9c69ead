"""Verify passes under the temperature / top-p sampler, the parts that need no GPU: the exported symbols, the refusals in front of any launch, the
CLI's Q4_SPECULATIVE_SAMPLED text, and the coin bookkeeping of the token loop around a pass against the library's own coin stream."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import spec_sampled_ref as ref
from llama_cu_awq_amd import api

ERR_ARG = 5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["q4_set_speculative_sampled", "q4_get_speculative_sampled", "q4_parse_speculative_sampled", "q4_verify_tokens_sampled", "q4_verify_covers_sampled",
       "q4_verify_sample_rows", "q4_verify_accept_tokens"]


def test_symbols_in_header_map_and_library():
    header = open(os.path.join(ROOT, "include", "llama2_q4.h")).read()
    exports = open(os.path.join(ROOT, "llama_cu_awq_amd", "csrc", "exports.map")).read()
    patterns = re.findall(r"[\w*]+(?=;)", exports.split("global:")[1].split("local:")[0])
    L = api.lib()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert any(re.fullmatch(p.replace("*", r"\w*"), name) for p in patterns), name
        assert hasattr(L, name) and name in api.SYMBOLS, name


def test_null_handles_and_bad_arguments_are_refused():
    L = api.lib()
    x = C.c_int(-5)
    d = (C.c_int * 1)(3)
    out = (C.c_int * 2)()
    assert L.q4_set_speculative_sampled(None, 1) == ERR_ARG
    assert L.q4_get_speculative_sampled(None) == 0
    assert L.q4_verify_covers_sampled(None, None, 0, 1) == 0
    assert L.q4_verify_tokens_sampled(None, None, d, 1, out, C.byref(x)) == ERR_ARG and x.value == -5
    coins = (C.c_float * 8)()
    assert L.q4_verify_sample_rows(None, None, 512, 1, coins, None) == ERR_ARG
    assert L.q4_verify_accept_tokens(None, 520, 517, d, 1, None, None, 64, None, None, None, None, None, None) == ERR_ARG
    assert L.q4_verify_accept_tokens(None, 520, 517, None, 1, None, None, 64, None, None, None, None, None, None) == ERR_ARG


def test_cli_switch_text():
    """Q4_SPECULATIVE_SAMPLED is a variable of its own: "1" or "0", anything else is refused with the output untouched; Q4_SPECULATIVE's grammar has no
    such key"""
    L = api.lib()
    on = C.c_int(-5)
    assert L.q4_parse_speculative_sampled(b"1", C.byref(on)) == 0 and on.value == 1
    assert L.q4_parse_speculative_sampled(b"0", C.byref(on)) == 0 and on.value == 0
    on.value = -5
    for bad in (b"", b"2", b"on", b"yes", b"1 ", b" 1", b"11", b"-1", b"true", b"1,draft=4"):
        assert L.q4_parse_speculative_sampled(bad, C.byref(on)) == ERR_ARG and on.value == -5, bad
    assert L.q4_parse_speculative_sampled(None, C.byref(on)) == ERR_ARG
    assert L.q4_parse_speculative_sampled(b"1", None) == ERR_ARG
    d, g, m = C.c_int(), C.c_int(), C.c_int()
    assert L.q4_parse_speculative(b"draft=4,sampled=1", C.byref(d), C.byref(g), C.byref(m)) == ERR_ARG
    host = open(os.path.join(ROOT, "llama_cu_awq_amd", "csrc", "q4_host.cpp")).read()
    assert 'getenv("Q4_SPECULATIVE_SAMPLED")' in host and "q4_parse_speculative_sampled(" in host and "q4_set_speculative_sampled(" in host


def test_coin_stream_restatement_and_its_inverse():
    L = api.lib()
    L.random_f32.restype = C.c_float
    for seed in (1, 7, 1234, 0x9E3779B97F4A7C15):
        state = C.c_ulonglong(seed)
        mine = seed
        for _ in range(50):
            c, mine = ref.coin_of(mine)
            assert L.random_f32(C.byref(state)) == np.float32(c) and state.value == mine
    for k in (0, 2, 1 << 23, (1 << 24) - 1, 12345):
        state = C.c_ulonglong(ref.state_for_coin(k))
        assert L.random_f32(C.byref(state)) == np.float32(k / 16777216.0)
    assert np.float32(((1 << 24) - 1) / 16777216.0) == np.float32(0.99999994)


@pytest.mark.parametrize("seed", [7, 11])
def test_coin_bookkeeping_around_passes(seed):
    """D + 1 coins drawn into the ring, the stream rewound, m + 1 drawn once m is known: every position that ran sampled with the coin the run without
    passes draws for it, stale entries are rewritten before they are read, and the stream ends where that run's ends"""
    steps, n_prompt = 120, 17
    r = np.random.default_rng(seed)
    passes, pos = [], n_prompt - 1
    while pos < steps - 8:
        d = int(r.integers(1, 8))
        m = (0, d, d // 2)[len(passes) % 3]                  # none, all, some
        passes.append((pos, d, m))
        pos += m + 1 + int(r.integers(0, 3)) * 8
    a, b, state_a, state_b = ref.replay_coins(seed, n_prompt, passes, lambda pos: 8, steps)
    assert len(passes) >= 5 and any(p[2] == 0 for p in passes) and any(p[2] == p[1] for p in passes)
    assert all(b[i] == a[i] for i in range(steps))
    assert state_a == state_b
    # one pass alone: D + 1 entries, the stream m + 1 draws further
    ring, after = ref.pass_coins(seed, 40, 5, 2)
    assert sorted(ring) == list(range(40, 46)) and [ring[40 + i] for i in range(6)] == ref.draw(seed, 6)[0] and after == ref.draw(seed, 3)[1]
    assert ref.accept_tokens([4, 5, 6, 7], [4, 5, 9]) == 2 and ref.accept_tokens([4, 5], [9]) == 0 and ref.accept_tokens([4, 5], [4]) == 1
