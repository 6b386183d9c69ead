"""q4_set_pass_context (include/llama2_q4.h) without a GPU: the setting's surface, and the expected-pass arithmetic of
tests/pass_context_ref.py on cases worked by hand."""
import os
import re

import numpy as np

import pass_context_ref as ref
from conftest import ROOT


# ---- the surface ----------------------------------------------------------------------------------------------------------------------------------
def test_declared_and_exported():
    from llama_cu_awq_amd import api
    header = open(os.path.join(ROOT, "include", "llama2_q4.h")).read()
    assert re.search(r"\bvoid\s+q4_set_pass_context\s*\(\s*int\s+positions\s*\)\s*;", header)
    assert re.search(r"\bint\s+q4_get_pass_context\s*\(\s*void\s*\)\s*;", header)
    assert {"q4_set_pass_context", "q4_get_pass_context"} <= set(api.SYMBOLS)
    L = api.lib()
    assert hasattr(L, "q4_set_pass_context") and hasattr(L, "q4_get_pass_context")


def test_default_and_clamp():
    from llama_cu_awq_amd import api
    assert api.get_pass_context() == 256
    try:
        for value in (0, 100, 256, -5):
            api.set_pass_context(value)
            assert api.get_pass_context() == 256
        api.set_pass_context(2304)
        assert api.get_pass_context() == 2304
        api.set_pass_context(257)
        assert api.get_pass_context() == 257
    finally:
        api.set_pass_context(256)
    assert api.get_pass_context() == 256


# ---- the arithmetic -------------------------------------------------------------------------------------------------------------------------------
def test_bins():
    assert [ref.bin_end(p) for p in (0, 127, 255, 256, 511, 512, 1023, 1024, 2047, 2048, 2303)] == [256, 256, 256, 512, 512, 1024, 1024, 2048, 2048, 4096, 4096]
    assert [ref.graph_bin(s, 2304) for s in (1, 128, 129, 256, 257, 512, 513, 1025, 2048, 2049, 2304)] == [128, 128, 256, 256, 512, 512, 1024, 2048, 2048, 4096, 4096]
    assert ref.graph_bin(8193, 20000) == 20000 and ref.graph_bin(8192, 20000) == 8192
    # forms by position: graphs / eager bins go by the bin, no graphs by the step's own size
    assert [ref.form(p, 1, 2304) for p in (0, 255, 256, 511, 512, 1023, 1024, 2047, 2048, 2303)] == ["v", "v", 64, 64, 128, 128, 256, 256, 256, 256]
    assert [ref.form(p, 0, 2304) for p in (0, 255, 256, 510, 511, 512, 1023, 1024, 2303)] == ["v", "v", None, None, 64, 128, 128, 256, 256]


def test_default_bound_is_todays_rule():
    """bound 256: what tests/test_prompt_ingest_gpu.py's _expected_passes counts, for every prompt length and start it uses"""
    def today(n_prompt, start=0):
        m = max(0, min(n_prompt - 1, 256) - start)
        return m // 8 + (1 if m % 8 >= 2 else 0)
    for n_prompt in (2, 3, 8, 9, 17, 130, 140, 270, 300):
        for start in (0, 5):
            for bound in (256, 0):
                got = ref.prompt_passes(n_prompt, n_prompt + 6, bound, 300, start=start)
                assert len(got) == today(n_prompt, start), (n_prompt, start)
                assert all(pos + n <= 256 for pos, n in got)


def _segments(passes):
    return [(pos, pos + n) for pos, n in passes]


def test_prompt_passes_by_hand():
    S = 2304
    # a 2200-token prompt: prompt-only positions 0 .. 2198. Bins [0, 256): 32 passes, [256, 512): 32, [512, 1024): 64, [1024, 2048): 128, and
    # 2048 .. 2198 = 151 positions: 18 passes of eight and one of seven
    p = ref.prompt_passes(2200, 2206, S, S)
    assert len(p) == 32 + 32 + 64 + 128 + 19 and p[-1] == (2192, 7) and p[0] == (0, 8)
    # up to the bound, which is the context: prompt-only positions 0 .. 2302, the last bin's share 255 = 31 x 8 + 7
    p = ref.prompt_passes(2304, 2304, S, S)
    assert len(p) == 32 + 32 + 64 + 128 + 32 and p[-1] == (2296, 7)
    # last prompt-only position 510 / 511 / 512: 64 passes each -- 256 .. 510 is 31 passes of eight and one of seven, 512 alone is a step
    assert [len(ref.prompt_passes(n, n + 6, S, S)) for n in (512, 513, 514)] == [64, 64, 64]
    assert ref.prompt_passes(512, 518, S, S)[-1] == (504, 7) and ref.prompt_passes(514, 520, S, S)[-1] == (504, 8)
    # ... 1022 / 1023 / 1024
    assert [len(ref.prompt_passes(n, n + 6, S, S)) for n in (1024, 1025, 1026)] == [128, 128, 128]
    # a run resumed at 3 with the last prompt-only position 513: 3 .. 255 is 31 passes and one of five, 256 .. 511 is 32, 512 .. 513 one of two.
    # (A loop that let a pass reach across 256 or 512 would count 64: 511 positions in 63 passes of eight and one of seven.)
    p = ref.prompt_passes(515, 521, S, S, start=3)
    assert len(p) == 65 and (251, 5) in p and (256, 8) in p and p[-1] == (512, 2)
    for a, b in _segments(p):
        assert ref.bin_end(a) >= b
    # an intermediate bound: 900 prompt tokens, bound 700 -- 512 .. 699 is 23 passes of eight and one of four, nothing behind
    p = ref.prompt_passes(900, 906, 700, S)
    assert len(p) == 32 + 32 + 24 and p[-1] == (696, 4)
    # the bound is cut at the model's context
    assert ref.prompt_passes(290, 296, 100000, 300) == ref.prompt_passes(290, 296, 300, 300)
    p = ref.prompt_passes(300, 300, 100000, 300)
    assert p[-1] == (296, 3) and len(p) == 32 + 5 + 1
    # no graphs, 600 prompt tokens: 256 .. 510 run the one-block form (no pass), 511 is alone in its bin, 512 .. 598 is ten passes and one of seven
    p = ref.prompt_passes(600, 606, S, S, mode=0)
    assert len(p) == 32 + 11 and p[32] == (512, 8) and p[-1] == (592, 7)
    # `steps` cuts too
    assert ref.prompt_passes(600, 300, S, S)[-1] == (296, 4)
    # smaller passes
    assert len(ref.prompt_passes(17, 23, S, S, ingest=3)) == 5
    # ... above 256: 1040 prompt tokens in passes of five. [0, 256) and [256, 512): 51 passes each, the position in front of the end a step; [512, 1024):
    # 102 passes and one of two (1022, 1023); 1024 .. 1038: three. Passes of five from 256 and from 512 straddle the chunk ends 320 and 640
    p = ref.prompt_passes(1040, 1046, S, S, ingest=5)
    assert len(p) == 51 + 51 + 103 + 3 and (250, 5) in p and (256, 5) in p and (316, 5) in p and (506, 5) in p and (637, 5) in p
    assert (1022, 2) in p and p[-1] == (1034, 5) and [x for x in p if x[1] != 5] == [(1022, 2)]
    assert len(ref.prompt_passes(1040, 1046, S, S)) == 32 + 32 + 64 + 2 and ref.prompt_passes(1040, 1046, S, S)[-1] == (1032, 7)


def test_covers_by_hand():
    S = 2304
    c = lambda pos, d, bound=S: ref.covers(pos, d + 1, bound, S)
    assert c(1016, 7) and not c(1017, 7) and c(1017, 6)
    assert c(2296, 7) and not c(2297, 7)
    assert c(248, 7, 256) and not c(249, 7, 256) and c(254, 1, 256) and not c(255, 1, 256)
    assert not c(249, 7) and c(249, 6) and c(256, 7)
    assert not c(300, 1, 256) and c(692, 7, 700) and not c(693, 7, 700) and c(693, 6, 700)
    # no graphs: positions 256 .. 510 have no form a pass reproduces
    assert not ref.covers(300, 2, S, S, mode=0) and ref.covers(600, 8, S, S, mode=0) and not ref.covers(510, 2, S, S, mode=0)


def test_replay_by_hand():
    S = 2304
    run = np.arange(3, 3 + 1200) % 500 + 3            # any ring without an EOS
    oracle = lambda ring, room: run[len(ring):len(ring) + room]
    # a 16-token prompt, every draft right: passes at 15, 23, ..., 247 (seven drafts each), at 255 there is no room (one step), then 256, 264, ...
    stats, passes = ref.replay(run, 16, 1100, oracle, 7, lambda pos: 1, S, S)
    assert passes[0] == (15, 7, 7) and passes[29] == (247, 7, 7) and passes[30] == (256, 7, 7)
    assert all(ref.bin_end(pos) > pos + d for pos, d, _ in passes)
    assert passes[-1][0] + passes[-1][2] + 1 == 1100 and passes[-1][1] == 1100 - 1 - passes[-1][0]
    assert stats[1] == stats[2]
    # with the default bound the replay is tests/spec_ref.py's
    import spec_ref
    assert ref.replay(run, 16, 400, oracle, 7, lambda pos: 1, 256, S) == spec_ref.replay(run, 16, 400, oracle, 7, lambda pos: 1)
    # a drafter that is right twice and then wrong: advances by three, so it meets the ends 256, 512 and 1024 out of step and its drafts are shortened there
    def two_right(ring, room):
        d = [int(x) for x in run[len(ring):len(ring) + room]]
        return d[:2] + [d[2] + 1] + d[3:] if len(d) > 2 else d
    stats, passes = ref.replay(run, 16, 1100, two_right, 7, lambda pos: 1, S, S)
    by_pos = {pos: (d, m) for pos, d, m in passes}
    assert by_pos[249] == (6, 2) and by_pos[252] == (3, 2) and 255 not in by_pos and by_pos[256] == (7, 2)
    assert by_pos[508] == (3, 2) and 511 not in by_pos and by_pos[512] == (7, 2)
    assert by_pos[1022] == (1, 1) and by_pos[1024] == (7, 2)
