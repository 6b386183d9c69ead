"""The schedule of a batch pass with several prompt positions per slot (q4_batch_plan_rows, csrc/q4_batch.hip), held to the Python
restatement in tests/batch_prefill_cases.py, and what q4_batch_set_prefill / q4_batch_get_prefill / q4_batch_plan_rows refuse. The schedule is a pure
host function of the library, so nothing here needs a GPU."""
import ctypes as C
import itertools

import numpy as np
import pytest

import batch_prefill_cases as bp

ERR_ARG = 5
REMAINING = [0, 1, 2, 3, 9]          # n_prompt - 1 - pos: prompt-only positions in front of the slot (0: its next row generates)


@pytest.fixture(scope="module")
def api():
    from llama_cu_awq_amd import api as mod
    return mod


def _case(api, open_, pos, n_prompt, cap):
    total, rows = api.Batch.plan_rows(open_, pos, n_prompt, cap)
    want_total, want = bp.plan_rows_ref(open_, pos, n_prompt, cap)
    what = "open %s pos %s n_prompt %s cap %d" % (open_, pos, n_prompt, cap)
    assert (total, [int(r) for r in rows]) == (want_total, want), what
    assert total == sum(rows) <= bp.MAX_ROWS, what
    for s, o in enumerate(open_):
        if not o:
            assert rows[s] == 0, what
            continue
        assert rows[s] >= 1, what
        assert rows[s] <= max(1, min(cap, n_prompt[s] - pos[s])), what
    if cap == 1:
        assert [int(r) for r in rows] == [1 if o else 0 for o in open_], what
    return rows


@pytest.mark.parametrize("n_slots", [1, 2, 3, 4])
def test_plan_equals_the_restatement(api, n_slots):
    """every combination of open / closed and remaining prompt per slot, at every cap; positions at 0 and deep in a sequence"""
    states = [(0, 0)] + [(1, r) for r in REMAINING]           # (open, remaining); a closed slot's words do not matter
    n = 0
    for combo in itertools.product(states, repeat=n_slots):
        for base in (0, 1000):
            open_ = [o for o, _ in combo]
            pos = [base + 3 * s for s in range(n_slots)]
            n_prompt = [pos[s] + 1 + r for s, (_, r) in enumerate(combo)]
            for cap in range(1, 9):
                _case(api, open_, pos, n_prompt, cap)
                n += 1
    assert n == len(states) ** n_slots * 2 * 8


def test_plan_with_eight_slots(api):
    eight = [1] * 8
    # a full batch has no row to spare, whatever the prompts
    assert list(_case(api, eight, [0] * 8, [50] * 8, 8)) == [1] * 8
    # spare rows go in slot order and run out
    assert list(_case(api, [1, 0, 1, 0, 1, 0, 0, 0], [0, 0, 0, 0, 0, 0, 0, 0], [50] * 8, 8)) == [6, 0, 1, 0, 1, 0, 0, 0]
    assert list(_case(api, [1, 0, 1, 0, 1, 0, 0, 0], [0, 0, 0, 0, 0, 0, 0, 0], [50] * 8, 3)) == [3, 0, 3, 0, 2, 0, 0, 0]
    # decoding slots (pos >= n_prompt - 1) take one; a slot two in front of its prompt's end takes its generating row too
    assert list(_case(api, [1, 1, 1, 1, 0, 0, 0, 1], [9, 20, 7, 0, 0, 0, 0, 3], [10, 5, 9, 2, 0, 0, 0, 40], 8)) == [1, 1, 2, 2, 0, 0, 0, 2]
    assert list(_case(api, [0] * 8, [0] * 8, [5] * 8, 4)) == [0] * 8
    rng = np.random.default_rng(5)
    for _ in range(300):
        open_ = [int(x) for x in rng.integers(0, 2, size=8)]
        pos = [int(x) for x in rng.integers(0, 2000, size=8)]
        n_prompt = [p + 1 + int(r) for p, r in zip(pos, rng.choice(REMAINING + [40], size=8))]
        _case(api, open_, pos, n_prompt, int(rng.integers(1, 9)))


def test_plan_refuses_bad_arguments(api):
    L = api.lib()
    three = (C.c_int * 3)(1, 1, 1)
    out = (C.c_int * 3)(7, 7, 7)
    for n_slots, cap in ((0, 1), (9, 1), (-1, 1), (3, 0), (3, 9), (3, -2)):
        assert L.q4_batch_plan_rows(three, three, three, n_slots, cap, out) == -ERR_ARG
    for args in ((None, three, three, 3, 1, out), (three, None, three, 3, 1, out), (three, three, None, 3, 1, out), (three, three, three, 3, 1, None)):
        assert L.q4_batch_plan_rows(*args) == -ERR_ARG
    assert list(out) == [7, 7, 7]


def test_set_prefill_refuses_without_a_batch(api):
    """the refusals that need no batch (the ones on a built batch: tests/test_batch_prefill_gpu.py)"""
    L = api.lib()
    assert L.q4_batch_set_prefill(None, 4) == ERR_ARG and L.q4_batch_get_prefill(None) == -ERR_ARG
