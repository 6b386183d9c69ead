"""Logit stages inside verify passes and the guide's forced drafts (q4_set_pass_stages; DESIGN.md 3.8 "Under the logit stages"), the parts that need no GPU:
the exported symbols, the CLI switch's text, the switch on handles the library did not build, the row entries' refusals in front of any launch, and
guide.forced_run -- the restatement of q4_guide_forced_run -- on tables worked out by hand."""
import ctypes as C
import os
import re

import numpy as np

from llama_cu_awq_amd import api, guide

ERR_ARG = 5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["q4_set_pass_stages", "q4_get_pass_stages", "q4_parse_pass_stages", "q4_guide_mask_rows", "q4_dry_penalty_rows", "q4_process_logits_rows",
       "q4_guide_forced_run", "q4_spec_stats_forced"]
DEAD, NONE, OFFTRACK = guide.DEAD, guide.NONE, guide.OFFTRACK


def test_symbols_in_header_map_and_library():
    header = open(os.path.join(ROOT, "include", "llama2_q4.h")).read()
    exports = open(os.path.join(ROOT, "llama_cu_awq_amd", "csrc", "exports.map")).read()
    patterns = re.findall(r"[\w*]+(?=;)", exports.split("global:")[1].split("local:")[0])
    L = api.lib()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert any(re.fullmatch(p.replace("*", r"\w*"), name) for p in patterns), name
        assert hasattr(L, name) and name in api.SYMBOLS, name


def test_cli_switch_text():
    """q4_parse_pass_stages: "1" and "0", nothing else; a refused text leaves *on alone (q4_parse_pass_gqa's contract)"""
    L = api.lib()
    on = C.c_int(7)
    assert L.q4_parse_pass_stages(b"1", C.byref(on)) == 0 and on.value == 1
    assert L.q4_parse_pass_stages(b"0", C.byref(on)) == 0 and on.value == 0
    on.value = 7
    for bad in (b"", b"2", b"1 ", b" 1", b"01", b"on", b"-1"):
        assert L.q4_parse_pass_stages(bad, C.byref(on)) == ERR_ARG and on.value == 7, bad
    assert L.q4_parse_pass_stages(None, C.byref(on)) == ERR_ARG
    assert L.q4_parse_pass_stages(b"1", None) == ERR_ARG


def test_switch_on_null_and_foreign_handles():
    L = api.lib()
    a, b = C.c_longlong(5), C.c_longlong(5)
    assert L.q4_set_pass_stages(None, 1) == ERR_ARG and L.q4_get_pass_stages(None) == 0
    assert L.q4_spec_stats_forced(None, C.byref(a), C.byref(b)) == ERR_ARG
    foreign = C.create_string_buffer(1 << 16)               # zeroed memory of a Transformer's size and more, which the library never built
    assert L.q4_set_pass_stages(foreign, 1) == ERR_ARG
    assert L.q4_set_pass_stages(foreign, 0) == ERR_ARG
    assert L.q4_get_pass_stages(foreign) == 0
    assert L.q4_spec_stats_forced(foreign, C.byref(a), C.byref(b)) == ERR_ARG and (a.value, b.value) == (5, 5)
    assert foreign.raw == bytes(1 << 16)                    # nothing was written through the handle


def test_row_entries_refuse_in_front_of_any_launch():
    """n_rows outside 1 .. 8, ld < n and ld & 7: Q4_ERR_ARG before anything is dereferenced or launched (the pointers are non-null and never read)"""
    L = api.lib()
    p = C.c_void_p(4096)
    dry = api.DryControls(multiplier=0.8)
    ctl = api.SamplingControls(top_k=4)
    for n_rows, ld, n in ((0, 520, 512), (-1, 520, 512), (9, 520, 512), (1 << 20, 520, 512), (3, 504, 512), (3, 511, 512), (3, 516, 512), (3, 0, 512), (3, -8, 512)):
        assert L.q4_dry_penalty_rows(p, n, C.byref(dry), None, 0, ld, n_rows, p, p) == ERR_ARG, (n_rows, ld, n)
        assert L.q4_process_logits_rows(p, n, C.byref(ctl), None, None, 0, ld, n_rows, p, p) == ERR_ARG, (n_rows, ld, n)
    assert L.q4_dry_penalty_rows(None, 512, C.byref(dry), None, 0, 520, 2, p, p) == ERR_ARG
    assert L.q4_dry_penalty_rows(p, 512, None, None, 0, 520, 2, p, p) == ERR_ARG
    assert L.q4_process_logits_rows(None, 512, C.byref(ctl), None, None, 0, 520, 2, p, p) == ERR_ARG
    assert L.q4_process_logits_rows(p, 512, None, None, None, 0, 520, 2, p, p) == ERR_ARG
    assert L.q4_process_logits_rows(p, 2, C.byref(ctl), None, None, 0, 8, 2, p, p) == ERR_ARG        # top_k above n
    assert L.q4_guide_mask_rows(p, 512, None, p, 520, 2, p, p) == ERR_ARG                             # no guide
    assert L.q4_guide_forced_run(None, 0, 4, p) == 0
    # neutral settings launch nothing, whatever the pointers
    assert L.q4_dry_penalty_rows(p, 512, C.byref(api.DryControls()), None, 0, 520, 2, p, p) == 0
    assert L.q4_process_logits_rows(p, 512, C.byref(api.SamplingControls()), None, None, 0, 520, 2, p, p) == 0


def test_python_surface():
    import inspect
    sig = inspect.signature(api.Transformer.__init__)
    assert sig.parameters["pass_stages"].default is False
    for name in ("set_pass_stages", "pass_stages", "spec_stats_forced"):
        assert callable(getattr(api.Transformer, name)), name
    for name in ("guide_mask_rows", "dry_penalty_rows", "process_logits_rows"):
        assert callable(getattr(api, name)), name
    assert callable(api.Guide.forced_run) and callable(guide.forced_run)


# ---- guide.forced_run by hand ---------------------------------------------------------------------------------------------------------------------------
def _trie():
    """from_choices([[5, 6, 7], [5, 8], [9]], 12): state 0 -{5}-> 1 -{6}-> 2 -{7}-> 3 (terminal); 1 -{8}-> 4 (terminal); 0 -{9}-> 5 (terminal); END = 6"""
    return guide.from_choices([[5, 6, 7], [5, 8], [9]], 12)


def test_forced_run_on_a_choices_trie():
    t = _trie()
    assert t.shape == (7, 12)
    assert guide.forced_run(t, 0, 7).tolist() == []                     # 5 or 9
    assert guide.forced_run(t, 1, 7).tolist() == []                     # 6 or 8
    assert guide.forced_run(t, 2, 7).tolist() == [7, 2]                 # the tail of the first choice, then EOS -- and the run ends behind it
    assert guide.forced_run(t, 3, 7).tolist() == [2]
    assert guide.forced_run(t, 4, 7).tolist() == [2]
    assert guide.forced_run(t, 6, 7).tolist() == [2]                    # END allows EOS alone: one token, not seven
    assert guide.forced_run(t, 2, 7).dtype == np.int32


def test_forced_run_stops_at_two_live_tokens_and_at_max_draft():
    # a chain 0 -> 1 -> 2 -> 3 -> 4 over tokens 10, 11, 12, 13; state 4 allows 3 and 4
    t = np.full((5, 16), DEAD, dtype=np.uint16)
    for s in range(4):
        t[s, 10 + s] = s + 1
    t[4, 3] = 0
    t[4, 4] = 4
    assert guide.forced_run(t, 0, 7).tolist() == [10, 11, 12, 13]
    assert guide.forced_run(t, 2, 7).tolist() == [12, 13]
    assert guide.forced_run(t, 4, 7).tolist() == []
    assert guide.forced_run(t, 0, 3).tolist() == [10, 11, 12]            # max_draft shorter than the run
    assert guide.forced_run(t, 0, 1).tolist() == [10]
    assert guide.forced_run(t, 0, 0).tolist() == []
    # a forced cycle never ends by itself: max_draft does
    c = np.full((2, 8), DEAD, dtype=np.uint16)
    c[0, 5] = 1
    c[1, 6] = 0
    assert guide.forced_run(c, 0, 7).tolist() == [5, 6, 5, 6, 5, 6, 5]
    # an EOS in the middle of a forced chain ends the run behind it
    e = np.full((3, 8), DEAD, dtype=np.uint16)
    e[0, 4] = 1
    e[1, 2] = 2
    e[2, 5] = 0
    assert guide.forced_run(e, 0, 7).tolist() == [4, 2]


def test_forced_run_on_states_that_are_none():
    t = _trie()
    for s in (NONE, OFFTRACK, 7, 4096, -7, 2 ** 31 - 1):
        assert guide.forced_run(t, s, 7).tolist() == [], s


def test_the_forced_drafts_case_is_forced_everywhere_behind_the_first_token():
    """what tests/test_pass_stages_gpu.py's forced-draft case relies on, on the CPU: 8 choices of 20 tokens that share their first token only -- state 0 is
    forced (that token), the state behind it has 8 live tokens, and every state behind a choice's second token is forced up to and including the EOS"""
    import pass_stages_cases as cases
    seqs = cases.forced_choices(8, 20)
    t = guide.from_choices(seqs, 512)
    assert guide.forced_run(t, 0, 7).tolist() == [seqs[0][0]]
    s1 = int(t[0, seqs[0][0]])
    assert int((t[s1] != DEAD).sum()) == 8 and guide.forced_run(t, s1, 7).tolist() == []
    for seq in seqs:
        states = guide.walk(t, seq)
        for j in range(2, len(seq) + 1):                                # behind token j - 1 (0-based), j >= 2
            want = list(seq[j:]) + [2]
            assert guide.forced_run(t, int(states[j]), 64).tolist() == want, (seq[:2], j)
