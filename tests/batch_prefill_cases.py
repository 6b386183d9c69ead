"""Helpers of tests/test_batch_prefill_host.py and tests/test_batch_prefill_gpu.py (several prompt positions of a slot per batch pass: q4_batch_set_prefill,
q4_batch_plan_rows; csrc/q4_batch.hip): a Python restatement of the schedule, a host-side tracker that follows every slot's position
through the passes with it, and the comparison of a slot with the run alone keyed on POSITIONS (batch_cases.assert_slot_equals assumes one per pass)."""
import numpy as np

import batch_cases as bc

MAX_ROWS = 8              # Q4_BATCH_MAX_SLOTS: the rows of a pass


def plan_rows_ref(open_, pos, n_prompt, cap):
    """q4_batch_plan_rows restated: one row per open slot; then, in slot order, the spare rows to the slots with pos < n_prompt - 1, each up to
    min(cap, n_prompt - pos) rows in all. Returns (rows in the pass, [rows per slot])."""
    rows = [1 if o else 0 for o in open_]
    spare = MAX_ROWS - sum(rows)
    for s in range(len(rows)):
        if not open_[s] or pos[s] < 0 or pos[s] >= n_prompt[s] - 1:
            continue
        extra = min(min(cap, n_prompt[s] - pos[s]) - 1, spare)
        rows[s] += extra
        spare -= extra
    return sum(rows), rows


class Tracker:
    """What the host knows of a batch without reading anything back: per slot open / position / prompt length, moved pass by pass by the restated plan.
    tokens[slot]: [(ring position, token)] of every token the slot generated; runs[slot]: [(first position, rows)] of every pass it took part in."""

    def __init__(self, n_slots):
        self.n = n_slots
        self.open = [False] * n_slots
        self.pos = [0] * n_slots
        self.n_prompt = [0] * n_slots
        self.tokens = [[] for _ in range(n_slots)]
        self.runs = [[] for _ in range(n_slots)]

    def opened(self, slot, n_prompt, pos=0):
        self.open[slot], self.pos[slot], self.n_prompt[slot] = True, pos, n_prompt
        self.tokens[slot], self.runs[slot] = [], []

    def closed(self, slot):
        self.open[slot] = False

    def plan(self, cap):
        return plan_rows_ref(self.open, self.pos, self.n_prompt, cap)[1]

    def passed(self, out_row, cap):
        """one pass ran at `cap`: out_row is its tokens_out [MAX_ROWS]"""
        rows = self.plan(cap)
        for s in range(self.n):
            if not rows[s]:
                assert out_row[s] == -1, "slot %d took no row and reports token %d" % (s, out_row[s])
                continue
            self.runs[s].append((self.pos[s], rows[s]))
            self.pos[s] += rows[s]
            if self.pos[s] >= self.n_prompt[s]:
                assert out_row[s] >= 0, "slot %d passed its prompt's end (position %d) without a token" % (s, self.pos[s])
                self.tokens[s].append((self.pos[s], int(out_row[s])))
            else:
                assert out_row[s] == -1, "slot %d is inside its prompt at %d and reports token %d" % (s, self.pos[s], out_row[s])
        assert (np.asarray(out_row[self.n:]) == -1).all()

    def passed_all(self, out, cap):
        for row in out:
            self.passed(row, cap)

    def ahead(self, passes, cap):
        """the positions after `passes` more passes at `cap`, this tracker left as it is"""
        pos = list(self.pos)
        for _ in range(passes):
            rows = plan_rows_ref(self.open, pos, self.n_prompt, cap)[1]
            pos = [p + r for p, r in zip(pos, rows)]
        return pos


def assert_slot_at(q4, batch, slot, solo, track, start, what, logits=True):
    """The slot that stood at `start` when `track` began to follow it, against the run alone that ran to the slot's position: the device position, every
    generated token by its ring position, the K / V rows of every layer from solo.first_row on, the logits of the last position -- bytes."""
    end = track.pos[slot]
    assert end == solo.steps, "%s: the slot ran to position %d, the run alone to %d" % (what, end, solo.steps)
    assert batch.pos(slot) == end, "%s: device position %d, expected %d" % (what, batch.pos(slot), end)
    n_prompt = len(solo.prompt)
    want = [(q, int(solo.tokens[q])) for q in range(max(start + 1, n_prompt), end + 1)]
    got = track.tokens[slot]
    assert [q for q, _ in got] == [q for q, _ in want], "%s: tokens at positions %s, expected at %s" % (what, [q for q, _ in got], [q for q, _ in want])
    assert got == want, "%s: tokens differ: %s vs the run alone %s" % (what, got, want)
    k, v = bc.slot_rows(q4, batch, slot, solo.first_row, end - solo.first_row)
    for name, a, b in (("K", k, solo.k), ("V", v, solo.v)):
        assert a.shape == b.shape, (what, name, a.shape, b.shape)
        bad = np.argwhere((a != b).any(axis=2))
        assert bad.size == 0, "%s: %s rows differ, first (layer, position) %s" % (what, name, [(int(x), int(y) + solo.first_row) for x, y in bad[:8]])
    if logits:
        mine = batch.logits(slot).view(np.uint16)
        assert np.array_equal(mine, solo.logits), "%s: final logits differ in %d entries" % (what, int((mine != solo.logits).sum()))
