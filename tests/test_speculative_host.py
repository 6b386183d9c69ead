"""Speculative greedy decoding, the parts that need no GPU (include/llama2_q4.h, csrc/spec_verify.h): the built-in prompt-lookup drafter against its
restatement (tests/spec_ref.py), the option text, the exported symbols, and that a null Transformer is refused."""
import ctypes as C
import itertools

import numpy as np
import pytest

import spec_ref
from llama_cu_awq_amd import api

ERR_ARG = 5
NEW = ["q4_verify_tokens", "q4_verify_covers", "q4_set_speculative", "q4_get_speculative", "q4_parse_speculative", "q4_set_drafter", "q4_spec_draft",
       "q4_spec_stats", "q4_verify_classifier", "q4_verify_accept"]

SETTINGS = [(d, g, m) for d, g in itertools.product((1, 4, 7), (1, 3)) for m in sorted({1, g})]


def test_symbols_are_exported():
    L = api.lib()
    for name in NEW:
        assert hasattr(L, name), name
        assert name in api.SYMBOLS


@pytest.mark.parametrize("max_draft,ngram_max,ngram_min", SETTINGS)
def test_draft_against_restatement(max_draft, ngram_max, ngram_min):
    """random rings over five symbols (matches abound), every length 1 .. 40, three rings per length"""
    r = np.random.default_rng(100 * max_draft + 10 * ngram_max + ngram_min)
    hits = 0
    for n in range(1, 41):
        for _ in range(3):
            ring = r.integers(0, 5, size=n)
            got = api.spec_draft(ring, max_draft, ngram_max, ngram_min)
            want = spec_ref.draft(ring, max_draft, ngram_max, ngram_min)
            assert got == want, (ring.tolist(), got, want)
            hits += bool(got)
    assert 8 < hits < 120          # of 120 rings: both outcomes occur at every setting (3-grams alone match least often)


def test_draft_cases():
    # the most recent earlier occurrence wins, and the longest n-gram is tried first
    ring = [7, 1, 2, 3, 9, 1, 2, 3, 8, 5, 2, 3]
    assert api.spec_draft(ring, 4, 3, 1) == [8, 5, 2, 3]               # "2 3" (no 3-gram "5 2 3" earlier): behind its latest earlier occurrence
    assert api.spec_draft(ring, 2, 3, 1) == [8, 5]
    assert api.spec_draft(ring, 4, 1, 1) == [8, 5, 2, 3]               # "3" alone: the same place
    assert api.spec_draft([1, 2, 3, 4, 1, 2, 3], 7, 3, 3) == [4, 1, 2, 3]          # the continuation runs into the tail itself and off the end
    assert api.spec_draft([5, 5, 5], 7, 2, 1) == [5]                   # overlapping occurrence: one token is left behind it
    assert api.spec_draft([4, 4], 7, 3, 1) == [4]
    # no match: a fresh last token; an n-gram range that is longer than anything repeated
    assert api.spec_draft([1, 2, 3, 4], 4, 3, 1) == []
    assert api.spec_draft([1, 2, 1, 3, 1, 2], 4, 3, 3) == []
    assert api.spec_draft([1], 4, 3, 1) == []
    for ring, d, g, m in (([1, 2, 3, 4, 1, 2, 3], 7, 3, 3), ([5, 5, 5], 7, 2, 1), ([1, 2, 3, 4], 4, 3, 1), (ring, 4, 3, 1)):
        assert api.spec_draft(ring, d, g, m) == spec_ref.draft(ring, d, g, m)


def test_draft_bad_arguments_give_nothing():
    L = api.lib()
    out = (C.c_int * 8)()
    ring = (C.c_int * 4)(1, 2, 1, 2)
    assert L.q4_spec_draft(None, 4, 4, 3, 1, out) == 0
    assert L.q4_spec_draft(ring, 4, 4, 3, 1, None) == 0
    assert L.q4_spec_draft(ring, 4, 0, 3, 1, out) == 0
    assert L.q4_spec_draft(ring, 4, 4, 1, 2, out) == 0
    assert L.q4_spec_draft(ring, 4, 4, 3, 0, out) == 0
    assert L.q4_spec_draft(ring, 4, 4, 3, 1, out) == 2 and list(out[:2]) == [1, 2]


def test_option_text():
    assert api.parse_speculative("draft=4,ngram=3,min=2") == {"draft": 4, "ngram": 3, "min": 2}
    assert api.parse_speculative("min=1,draft=7,ngram=8") == {"draft": 7, "ngram": 8, "min": 1}
    assert api.parse_speculative("draft=2") == {"draft": 2, "ngram": 3, "min": 2}          # the defaults: draft=4, ngram=3, min=2
    assert api.parse_speculative("ngram=5") == {"draft": 4, "ngram": 5, "min": 2}
    assert api.parse_speculative("ngram=1") == {"draft": 4, "ngram": 1, "min": 1}
    assert api.parse_speculative("draft=0")["draft"] == 0
    L = api.lib()
    d, g, m = C.c_int(-5), C.c_int(-5), C.c_int(-5)
    for bad in ("draft=8", "draft=4,ngram=9", "draft=4,ngram=2,min=3", "draft=4,min=0", "draft", "draft=", "draft=4,", "drafts=4", "draft=-1", "draft= 4",
                "draft=4x", "draft=4;ngram=3"):
        assert L.q4_parse_speculative(bad.encode(), C.byref(d), C.byref(g), C.byref(m)) == ERR_ARG, bad
        assert (d.value, g.value, m.value) == (-5, -5, -5), bad
    assert L.q4_parse_speculative(None, C.byref(d), C.byref(g), C.byref(m)) == ERR_ARG
    assert L.q4_parse_speculative(b"draft=4", None, C.byref(g), C.byref(m)) == ERR_ARG


def test_null_transformer_is_refused():
    L = api.lib()
    x = C.c_int()
    assert L.q4_set_speculative(None, 4, 3, 1) == ERR_ARG
    assert L.q4_get_speculative(None, C.byref(x), C.byref(x), C.byref(x)) == ERR_ARG
    assert L.q4_set_drafter(None, api.DRAFTER_FN(), None) == ERR_ARG
    assert L.q4_spec_stats(None, None, None, None) == ERR_ARG
    assert L.q4_verify_covers(None, 0, 1) == 0
    d = (C.c_int * 1)(3)
    out = (C.c_int * 2)()
    assert L.q4_verify_tokens(None, d, 1, out, C.byref(x)) == ERR_ARG
    assert L.q4_status_string(api.NOT_ADMITTED) == b"not admitted"
