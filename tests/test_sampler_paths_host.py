"""The inputs of tests/test_sampler_paths_gpu.py, classified on the CPU (tests/sampler_paths_ref.py): every branch of topp_sample_kernel that a
vocabulary size can reach must receive at least MIN_PER_LABEL of that size's trials, with the coins the GPU test will draw. A condition on the INPUTS:
a label that falls short wants more cases in sampler_paths_ref.cases, not a lower count. The census goes to profiles/sampler_paths_census.json. Also
here: the oracle's token always has a finite input logit (a -inf entry has probability 0 and is never the sample)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import sampler_paths_ref as ref
from conftest import ROOT
from llama_cu_awq_amd import api

MIN_PER_LABEL = 8
SEED = 99
CENSUS = os.path.join(ROOT, "profiles", "sampler_paths_census.json")

# What each size can reach, read off the kernel's conditions. E = ceil(n / 1024); `need` = threshold x 1.01 + 0.004 with the threshold = coin x topp,
# so at the settings these tests run (topp 0.9 and 0.6) `need` stays below 0.913; b0 .. b3 are the masses of the band lists (entries >= 2^-9,
# [2^-10, 2^-9), [2^-11, 2^-10), [2^-12, 2^-11)), n0 .. n3 their sizes. EVERY label listed must hold MIN_PER_LABEL trials, and a label that is not
# listed fails the test when it turns up. What is not listed, and why it cannot happen:
#  * n > 32768, the global-memory form: sorted or not, nothing else -- its softmax hands back no top entry, so there is no shortcut, and it has
#    neither lists nor cuts. (128256 / 128259: the same two; there every finite logit, and so every token the restatement draws, has an id >= 65536.)
#  * the block's scan wants ceil(m / E) > 64 with m <= 1024: E <= 15, so not from 16384 on; with one list m = n0 <= 512 (512 x 2^-9 = 1): E <= 7, so
#    not at 8192; at n = 64 m <= 64 = 64 E.
#  * `overflow` (a band list above 1024 entries) and `wide` (m > 1024) want more than 1024 finite entries: not up to n = 1024. Only bands 2 and 3
#    can overflow (512 and 1024 entries fill bands 0 and 1 to a mass of 1).
#  * `too-many` wants more than 4096 probabilities >= 2^-12, which sum to more than 1 unless they ARE 2^-12 after rounding: 4097 equal entries
#    (1 / 4097 rounds UP to 2^-12). So n >= 4097, band 3 overflows with it (never `wide/` or `short/`), and nothing else gets there.
#  * `wide` takes three or four lists (n0 + n1 <= 1024 since n0 2^-9 + n1 2^-10 <= 1), so b0 < need and the cut 2^-9 does not cover; the lists taken
#    do cover, so the cut 2^-11 (three lists) or 2^-12 (four) does: `wide/cut11`, `wide/cut12` and no other.
#  * `short` (the four lists together do not cover `need`) sums the same entries the cut 2^-12 sums: `short/none` and no other. (Two fp32 sums of
#    the same entries in another order could disagree in the last bit; no input here sits there.)
#  * n = 64: what the first two lists leave, at least 1 - 0.913 of the mass, would have to lie in at most 63 entries below 2^-10, which hold less
#    than 0.062: no third or fourth list, no `short`. Two lists are reachable (63 entries below 2^-9 hold up to 0.123).
_TOP = ["pre/top-alone", "pre/scan/scalar"]
_WAVE0 = ["pre/lists%d/wave0" % k for k in (1, 2, 3, 4)]
_BLOCK = ["pre/lists%d/block" % k for k in (2, 3, 4)]
_OVERFLOW = ["pre/overflow/cut9", "pre/overflow/cut11", "pre/overflow/cut12", "pre/overflow/none"]
_WIDE = ["pre/wide/cut11", "pre/wide/cut12"]
_E1 = _TOP + _WAVE0 + ["pre/lists1/block"] + _BLOCK + ["pre/short/none"]
_LARGE = _TOP + _WAVE0 + _OVERFLOW + ["pre/overflow/too-many"] + _WIDE + ["pre/short/none"]
_LARGE_32 = [s.replace("scan/scalar", "scan/vector") for s in _LARGE]
_ONE_BLOCK = ["one-block/top-alone", "one-block/scan/scalar", "one-block/cut9", "one-block/cut11", "one-block/cut12", "one-block/none"]
REACHABLE = {
    64: _TOP + ["pre/lists1/wave0", "pre/lists2/wave0"],
    1000: _E1,
    1001: _ONE_BLOCK,
    1024: _E1,
    2048: _E1 + _OVERFLOW + _WIDE,
    8192: _LARGE + _BLOCK,
    16384: _LARGE,
    16392: _LARGE,
    20000: _LARGE,
    32000: _LARGE_32,
    32003: _ONE_BLOCK + ["one-block/too-many"],
    32768: _LARGE_32,
    32776: ["global/sort", "global/scan"],
    40000: ["global/sort", "global/scan"],
    128256: ["global/sort", "global/scan"],
    128259: ["global/sort", "global/scan"],
}


@pytest.fixture(scope="module")
def census():
    return {}


def test_the_size_lists_agree():
    assert set(REACHABLE) == set(ref.SIZES)
    for n in ref.SIZES:
        E = (n + 1023) // 1024
        assert 1 <= E <= 126


@pytest.mark.parametrize("n", ref.SIZES)
def test_every_reachable_branch_holds_enough_trials(orc, census, n):
    L, O = api.lib(), orc.lib()
    state = C.c_ulonglong(SEED)
    count = {}
    toks = []
    for name, x, T, topp, coin_range in ref.trials(n):
        _, coin = ref.next_coin(L.random_f32, state, coin_range)      # the stream the GPU test's sampler draws
        label = ref.classify(x, n, T, topp, coin)
        count[label] = count.get(label, 0) + 1
        tok = O.orc_sample_topp(orc.f16_bits(x.copy()), n, T, topp, coin)
        assert 0 <= tok < n and np.isfinite(np.float32(x[tok])), "%s: the restatement's token %d has logit %r (%s)" % (name, tok, x[tok], label)
        assert tok >= ref.low_id(n) and int(np.flatnonzero(np.isfinite(x.astype(np.float32))).min()) >= ref.low_id(n), name
        toks.append(tok)
    assert n <= ref.HIGH or max(toks) > 98304, max(toks)
    census[str(n)] = dict(sorted(count.items()))
    print("n %d: %s" % (n, census[str(n)]))
    short = {k: count.get(k, 0) for k in REACHABLE[n] if count.get(k, 0) < MIN_PER_LABEL}
    assert not short, "n %d: labels below %d trials: %s -- add cases to sampler_paths_ref.cases" % (n, MIN_PER_LABEL, short)
    extra = sorted(set(count) - set(REACHABLE[n]))
    assert not extra, "n %d: labels the list of reachable ones says cannot happen: %s" % (n, extra)


@pytest.mark.parametrize("n,topp,supports", ref.FALLBACK)
def test_no_prefix_reaches_the_threshold(orc, n, topp, supports):
    """the restatement where the fp16 total stays below the coin: the last entry with a probability above 0, never the -inf logit at n - 1"""
    state = C.c_ulonglong(ref.FALLBACK_STATE)
    coin = api.lib().random_f32(C.byref(state))
    assert coin > 0.9999
    for k in supports:
        x, last = ref.fallback_case(n, k)
        assert np.isneginf(np.float32(x[n - 1]))
        assert orc.lib().orc_sample_topp(orc.f16_bits(x.copy()), n, 1.0, topp, coin) == last, (n, topp, k)


def test_the_committed_census_is_this_one(census):
    """runs behind the parametrised test and writes what it counted (a partial run, or a tree that cannot be written, leaves the committed file as
    it is); the file then shows at least MIN_PER_LABEL trials for every label listed above"""
    if set(census) == set(str(n) for n in ref.SIZES):
        try:
            with open(CENSUS, "w") as f:
                json.dump({"min_per_label": MIN_PER_LABEL, "seed": SEED, "trials": {n: sum(c.values()) for n, c in census.items()}, "census": census},
                          f, indent=1, sort_keys=True)
                f.write("\n")
        except OSError:
            pass
    with open(CENSUS) as f:
        doc = json.load(f)
    assert set(doc["census"]) == set(str(n) for n in ref.SIZES)
    for n in ref.SIZES:
        for label in REACHABLE[n]:
            assert doc["census"][str(n)].get(label, 0) >= doc["min_per_label"] >= MIN_PER_LABEL, (n, label)
