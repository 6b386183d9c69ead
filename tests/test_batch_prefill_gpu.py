"""Several prompt positions of a slot per batch pass (q4_batch_set_prefill; csrc/q4_batch.hip, the run form of the split-context attention in
csrc/prompt_pass.hip). The invariant is test_batch_gpu.py's, and there is no tolerance anywhere: what a slot produces -- its tokens, every
K / V row, the logits of its last position -- is BYTE for byte what the same checkpoint produces when it runs that sequence alone (q4_generate_ids on a
second Transformer of the same file, greedy screen off), whatever the other slots do and whichever pass carried a position.

  1. equality: 1, 2, 3, 5 and 8 slots with prompts of 1 .. 40 tokens, 64 passes, at caps 2, 5 and 8; the device positions follow the plan step by step;
  2. a lone slot: a 37-token prompt at cap 8 reaches its first token in ceil(37 / 8) passes;
  3. every attention form under runs: slots restored from snapshots on prompts 12 positions longer, among decoding slots, a run across 127 / 128, across
     every position at which the step's attention plan changes (with graphs and without) and across a chunk boundary of every chunk size; two runs in
     one launch; without graphs a run that would enter 256 .. 510 is refused, nothing moved;
  4. the temperature / top-p sampler with a seed per slot: the first sampled token behind a prompt ingested by runs shows where the coin stream stood;
  5. poisoned caches and churn; 6. the grouped-query shape; 7. a hostile checkpoint; 8. the cap changed between passes; 9. Batch.run with an eos;
  10. what q4_batch_set_prefill refuses on a built batch."""
import numpy as np
import pytest

import batch_cases as bc
import batch_prefill_cases as bp
import hostile_models as hm
import pass_context_ref as ref
from llama_cu_awq_amd import synth

pytestmark = pytest.mark.gpu

S = 2304                  # pass_long's and gqa7b_pair's context
PASSES = 64
LENGTHS = [1, 3, 8, 9, 17, 30, 37, 40]
PAST = 12                 # test 3: prompt positions behind the snapshot
UNSUPPORTED, ERR_ARG = 1, 5


@pytest.fixture(scope="module")
def checkpoints(tmp_path_factory):
    d = tmp_path_factory.mktemp("batch_prefill")
    made = {}

    def get(name):
        if name not in made:
            path = str(d / (name.replace("/", "_") + ".bin"))
            if "/" in name:
                hm.write_hostile_model(path, *name.split("/"), seed=7)
            else:
                synth.write_model(path, name, seed=31)
            made[name] = path
        return made[name]
    return get


@pytest.fixture(scope="module")
def pairs(q4, checkpoints):
    """(the batch's Transformer, the one that runs alone) per checkpoint, with the greedy screen off while the module runs"""
    L = q4.lib()
    screen = L.q4_get_greedy_screen()
    L.q4_set_greedy_screen(0)
    made = {}

    def get(name):
        if name not in made:
            made[name] = (q4.Transformer(checkpoints(name)), q4.Transformer(checkpoints(name)))
        return made[name]
    yield get
    for a, b in made.values():
        a.close()
        b.close()
    L.q4_set_greedy_screen(screen)


_solo = {}


def _alone(q4, t, name, prompt_tokens, steps, first_row=0, key=""):
    k = (name, tuple(prompt_tokens), steps, first_row, key)
    if k not in _solo:
        _solo[k] = bc.Solo(q4, t, prompt_tokens, steps, first_row)
    return _solo[k]


def _equality(q4, pairs, name, n_slots, lengths, cap, passes=PASSES):
    a, b = pairs(name)
    batch = q4.Batch(a, n_slots, prefill_rows=cap)
    try:
        assert batch.prefill() == cap
        track = bp.Tracker(n_slots)
        prompts = [bc.prompt(lengths[i], seed=100 + i) for i in range(n_slots)]
        for i, p in enumerate(prompts):
            batch.open(i, p)
            track.opened(i, len(p))
        out = batch.generate(passes)
        assert out.shape == (passes, q4.BATCH_MAX_SLOTS)
        track.passed_all(out, cap)
        if n_slots < q4.BATCH_MAX_SLOTS and max(lengths[:n_slots]) > 2:
            assert any(n > 1 for runs in track.runs for _, n in runs), "no slot ever took more than one row"
        for i, p in enumerate(prompts):
            bp.assert_slot_at(q4, batch, i, _alone(q4, b, name, p, track.pos[i]), track, 0, "%s, %d slots, cap %d, slot %d" % (name, n_slots, cap, i))
    finally:
        batch.delete()


# ---- 1. equality ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap", [2, 5, 8])
@pytest.mark.parametrize("n_slots", [1, 2, 3, 5, 8])
def test_slots_equal_their_runs_alone(q4, pairs, n_slots, cap):
    _equality(q4, pairs, "pass_long", n_slots, LENGTHS, cap)


def test_device_positions_follow_the_plan(q4, pairs):
    """q4_batch_step pass by pass: after every pass the position on the device is the one the restated plan gives, and the tokens are the run alone's"""
    a, b = pairs("pass_long")
    lengths, cap = [9, 17, 3], 5
    prompts = [bc.prompt(n, seed=120 + n) for n in lengths]
    batch = q4.Batch(a, 3, prefill_rows=cap)
    try:
        track = bp.Tracker(3)
        for i, p in enumerate(prompts):
            batch.open(i, p)
            track.opened(i, len(p))
        assert track.plan(cap) == [5, 2, 1]                      # five spare rows: four to slot 0, the last to slot 1
        for _ in range(10):
            track.passed(batch.step(), cap)
            assert [batch.pos(i) for i in range(3)] == track.pos
        for i, p in enumerate(prompts):
            bp.assert_slot_at(q4, batch, i, _alone(q4, b, "pass_long", p, track.pos[i]), track, 0, "step by step, slot %d" % i)
    finally:
        batch.delete()


# ---- 2. a lone slot -------------------------------------------------------------------------------------------------------------------------------------
def test_a_lone_slot_ingests_eight_positions_per_pass(q4, pairs):
    a, b = pairs("pass_long")
    p = bc.prompt(37, seed=137)
    batch = q4.Batch(a, 1, prefill_rows=8)
    try:
        track = bp.Tracker(1)
        batch.open(0, p)
        track.opened(0, len(p))
        for i in range(5):                                       # ceil(37 / 8)
            out = batch.step()
            track.passed(out, 8)
            assert batch.pos(0) == min(8 * (i + 1), 37)
            assert (out[0] >= 0) == (i == 4)
        solo = _alone(q4, b, "pass_long", p, 37)
        assert out[0] == solo.tokens[37]
        bp.assert_slot_at(q4, batch, 0, solo, track, 0, "a lone slot")
    finally:
        batch.delete()


# ---- 3. every attention form under runs -----------------------------------------------------------------------------------------------------------------
def _boundaries(mode):
    """[(position a run must straddle, where the slot starts)]: 128; every position at which the plan of the step's attention changes (the form, the chunk
    size or -- with graphs -- the bin argument); a chunk boundary inside the range of every chunk size.
    Without graphs (mode 0) the step's bin argument is pos + 1 itself, and two of the named cases do not exist there -- they are accounted for, not dropped:
      * the computed edges are 256, 511, 512 and 1024. Positions 256 .. 510 have no row form, so no run can stand below 256 and cross it, nor cross 511:
        entering them is test_a_run_without_a_row_form_is_refused's case. 512 is crossed by a run that starts at 511, the first position with a form;
        128 and 2048 are not plan changes without graphs and are crossed all the same, as the positions the issue names;
      * chunks of 64 serve position 511 alone (bin argument 512), so there is no chunk boundary at chunk size 64 to cross: the chunk-boundary cases are
        those of 128 and 256, and chunk size 64 is run by the row at 511 in the run across 512."""
    def plan(pos):
        return ref.form(pos, mode, S), (ref.bin_arg(pos, mode, S) if mode else 0)
    edges = [pos for pos in range(1, S - 32) if plan(pos) != plan(pos - 1)]
    if mode:
        assert edges == [128, 256, 512, 1024, 2048], edges
    else:
        assert edges == [256, 511, 512, 1024], edges
        edges = [128, 512, 1024, 2048]                          # (the docstring says why)
    chunked = []
    for c in (64, 128, 256):
        e = next((pos for pos in range(c, S - 32, c) if all(plan(q) == plan(pos) and ref.form(q, mode, S) == c for q in range(pos - 4, pos + PAST + 4))), None)
        if e is not None:                                       # (without graphs chunks of 64 serve position 511 alone)
            chunked.append(e)
    assert len(chunked) == (3 if mode else 2), chunked
    cases = []
    for e in edges + chunked:
        s = e - 3
        while ref.form(s, mode, S) is None:                     # (no graphs, 512: the first position with a row form is 511)
            s += 1
        assert s < e
        cases.append((e, s))
    return cases


def _restored_case(q4, a, b, long_prompt, starts, n_decoders, cap, passes, straddle, what):
    """`n_decoders` slots that decode from their first pass (a one-token prompt) and one slot per start, restored there on a prompt PAST positions
    longer; every slot against its run alone. straddle: a position some run of two or more rows must contain together with the one below it."""
    snaps, runs = [], []
    n_slots = n_decoders + len(starts)
    batch = q4.Batch(a, n_slots, prefill_rows=cap)
    try:
        track = bp.Tracker(n_slots)
        deco = [[1] for _ in range(n_decoders)]
        for i, p in enumerate(deco):
            track.opened(i, 1)
        for j, s in enumerate(starts):
            track.opened(n_decoders + j, s + 1 + PAST, pos=s)
        ends = track.ahead(passes, cap)
        for j, s in enumerate(starts):
            runs.append(bc.Solo(q4, b, long_prompt[: s + 1 + PAST], ends[n_decoders + j], first_row=s))
            snaps.append(b.snapshot(s))
        for i, p in enumerate(deco):
            batch.open(i, p, seed=i + 1)
        for j, s in enumerate(starts):
            batch.restore(n_decoders + j, snaps[j], long_prompt[: s + 1 + PAST])
        out = batch.generate(passes)
        assert out.shape[0] == passes
        track.passed_all(out, cap)
        if straddle is not None:
            assert any(first < straddle <= first + n - 1 for j in range(len(starts)) for first, n in track.runs[n_decoders + j]), (what, track.runs)
        for i, p in enumerate(deco):
            bp.assert_slot_at(q4, batch, i, _alone(q4, b, "pass_long", p, ends[i]), track, 0, "%s, decoder %d" % (what, i))
        for j, s in enumerate(starts):
            bp.assert_slot_at(q4, batch, n_decoders + j, runs[j], track, s, "%s, restored at %d" % (what, s))
    finally:
        batch.delete()
        for s in snaps:
            s.close()


@pytest.mark.parametrize("mode", [1, 0])
def test_every_attention_form_under_runs(q4, pairs, mode):
    L = q4.lib()
    a, b = pairs("pass_long")
    long_prompt = bc.prompt(S, seed=200)
    L.q4_set_use_graphs(mode)
    try:
        for e, s in _boundaries(mode):
            # two decoders leave five spare rows: the restored slot takes runs of six, six and its generating row, then decodes
            _restored_case(q4, a, b, long_prompt, [s], 2, 8, 5, e, "graphs %d, across %d" % (mode, e))
    finally:
        L.q4_set_use_graphs(1)


def test_two_runs_in_one_launch(q4, pairs):
    """two slots inside their prompts in the same chunk-size list (positions 600 and 700: chunks of 128): runs of four and three rows in one launch"""
    a, b = pairs("pass_long")
    assert ref.form(600, 1, S) == ref.form(720, 1, S) == 128
    _restored_case(q4, a, b, bc.prompt(S, seed=200), [600, 700], 1, 4, 6, None, "two runs")


def test_a_run_without_a_row_form_is_refused(q4, pairs):
    """without graphs the step at positions 256 .. 510 runs the one-block form, which no pass restates: a run that would enter them refuses the whole
    pass in front of its first launch, and nothing moves"""
    L = q4.lib()
    a, b = pairs("pass_long")
    assert ref.form(255, 0, S) == "v" and ref.form(256, 0, S) is None
    p = bc.prompt(252 + 1 + PAST, seed=201)
    b.generate_ids(p, 260)
    snap = b.snapshot(252)
    batch = q4.Batch(a, 2, prefill_rows=8)
    try:
        batch.open(0, bc.prompt(4, seed=202))
        batch.restore(1, snap, p)
        L.q4_set_use_graphs(0)
        out = np.zeros(q4.BATCH_MAX_SLOTS, dtype=np.int32)
        assert q4.Batch.plan_rows([1, 1], [0, 252], [4, len(p)], 8)[1].tolist() == [4, 4]       # rows 252 .. 255: still admitted
        batch.set_prefill(8)
        assert L.q4_batch_step(batch.h, a.sampler, out.ctypes.data) == 0 and batch.pos(0) == 4 and batch.pos(1) == 256
        assert L.q4_batch_step(batch.h, a.sampler, out.ctypes.data) == UNSUPPORTED                 # rows 256 ..: no row form
        assert batch.pos(0) == 4 and batch.pos(1) == 256
        L.q4_set_use_graphs(1)
        assert batch.step()[1] == -1 and batch.pos(0) == 5 and batch.pos(1) == 263
    finally:
        L.q4_set_use_graphs(1)
        batch.delete()
        snap.close()


# ---- 4. the temperature / top-p sampler ----------------------------------------------------------------------------------------------------------------
def test_sampled_slots_equal_their_runs_alone(q4, pairs):
    a, b = pairs("pass_long")
    seeds, lengths, cap, passes = [21, 22, 23], [37, 9, 30], 5, 40
    prompts = [bc.prompt(n, seed=300 + n) for n in lengths]
    try:
        track = bp.Tracker(3)
        for i, p in enumerate(prompts):
            track.opened(i, len(p))
        ends = track.ahead(passes, cap)
        runs = []
        for p, seed, end in zip(prompts, seeds, ends):
            bc.set_sampler(q4, b, 0.5, 0.6, seed)
            runs.append(bc.Solo(q4, b, p, end))
        bc.set_sampler(q4, a, 0.5, 0.6, 999)        # (its own stream is not used: a slot's coins come from the slot's seed)
        batch = q4.Batch(a, 3, prefill_rows=cap)
        try:
            for i, (p, seed) in enumerate(zip(prompts, seeds)):
                batch.open(i, p, seed=seed)
            track.passed_all(batch.generate(passes), cap)
            for i, solo in enumerate(runs):
                # (the first token behind the prompt is drawn with coin number n_prompt - 1 of the slot's stream: a slot that drew one coin per PASS
                # while it ingested by runs would stand elsewhere in the stream and sample other tokens from there on)
                bp.assert_slot_at(q4, batch, i, solo, track, 0, "sampled, slot %d (seed %d)" % (i, seeds[i]))
            assert len({tuple(r.tokens[len(r.prompt):len(r.prompt) + 8]) for r in runs}) > 1     # (the seeds matter)
        finally:
            batch.delete()
    finally:
        bc.set_sampler(q4, a, 0.0, 0.9, 1)
        bc.set_sampler(q4, b, 0.0, 0.9, 1)


# ---- 5. poisoned caches and churn ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", ["nan", "huge"])
def test_churn_on_poisoned_caches(q4, pairs, pattern):
    a, b = pairs("pass_long")
    first, second, cap = 6, 9, 8
    prompts = [bc.prompt(n, seed=400 + n) for n in (23, 12, 2)]
    newcomer = bc.prompt(19, seed=444)
    batch = q4.Batch(a, 3, prefill_rows=cap)
    try:
        track = bp.Tracker(3)
        for slot in range(3):
            bc.poison_slot(q4, batch, slot, pattern)
        for slot, p in enumerate(prompts):
            batch.open(slot, p)
            track.opened(slot, len(p))
        track.passed_all(batch.generate(first), cap)
        # the prompts were ingested by runs: rows above each slot's end are still the pattern, everything below is the run alone's
        for slot, p in enumerate(prompts):
            assert any(n > 1 for _, n in track.runs[slot]) or len(p) <= 2
            bp.assert_slot_at(q4, batch, slot, _alone(q4, b, "pass_long", p, track.pos[slot]), track, 0, "%s, slot %d after %d passes" % (pattern, slot, first))
            bc.assert_poison_above(q4, batch, slot, track.pos[slot], pattern, "%s, slot %d after %d passes" % (pattern, slot, first))
        batch.close(1)
        track.closed(1)
        batch.open(1, newcomer)
        track.opened(1, len(newcomer))
        track.passed_all(batch.generate(second), cap)
        assert any(n > 1 for _, n in track.runs[1]), "the newcomer never took a run"
        for slot in (0, 2):
            bp.assert_slot_at(q4, batch, slot, _alone(q4, b, "pass_long", prompts[slot], track.pos[slot]), track, 0, "%s, survivor %d" % (pattern, slot))
            bc.assert_poison_above(q4, batch, slot, track.pos[slot], pattern, "%s, survivor %d" % (pattern, slot))
        bp.assert_slot_at(q4, batch, 1, _alone(q4, b, "pass_long", newcomer, track.pos[1]), track, 0, "%s, newcomer" % pattern)
    finally:
        batch.delete()


# ---- 6. grouped-query, 7. hostile weights ---------------------------------------------------------------------------------------------------------------
def test_grouped_query_slots_equal_their_runs_alone(q4, pairs):
    _equality(q4, pairs, "gqa7b_pair", 3, [2, 11, 33], 8)


def test_hostile_weights(q4, pairs):
    _equality(q4, pairs, "pass_long/combined", 3, [4, 19, 40], 5)


# ---- 8. the cap changed between passes ------------------------------------------------------------------------------------------------------------------
def test_cap_changed_between_passes(q4, pairs):
    a, b = pairs("pass_long")
    prompts = [bc.prompt(40, seed=800), bc.prompt(30, seed=801)]
    batch = q4.Batch(a, 2)
    try:
        track = bp.Tracker(2)
        for i, p in enumerate(prompts):
            batch.open(i, p)
            track.opened(i, len(p))
        assert batch.prefill() == 1
        for cap, passes in ((1, 3), (8, 2), (3, 25)):
            batch.set_prefill(cap)
            assert batch.prefill() == cap
            track.passed_all(batch.generate(passes), cap)
        assert track.runs[0][:6] == [(0, 1), (1, 1), (2, 1), (3, 7), (10, 7), (17, 3)] and track.runs[1][:6] == [(0, 1), (1, 1), (2, 1), (3, 1), (4, 1), (5, 3)]
        for i, p in enumerate(prompts):
            bp.assert_slot_at(q4, batch, i, _alone(q4, b, "pass_long", p, track.pos[i]), track, 0, "cap 1 -> 8 -> 3, slot %d" % i)
    finally:
        batch.delete()


# ---- 9. Batch.run ---------------------------------------------------------------------------------------------------------------------------------------
def test_run_serves_six_requests_through_three_slots(q4, pairs):
    a, b = pairs("pass_long")
    new = 12
    requests = [bc.prompt(n, seed=900 + n) for n in (21, 5, 33, 1, 14, 26)]
    alone = []
    for p in requests:
        toks = b.generate_ids(p, len(p) - 1 + new)[0]
        assert len(toks) == len(p) + new, "the run alone stopped early: pick another prompt"
        alone.append([int(x) for x in toks[len(p):]])
    # an eos the run alone is known to emit: the token most requests generate somewhere before their last one
    counts = {}
    for g in alone:
        for tok in set(g[:-1]):
            counts[tok] = counts.get(tok, 0) + 1
    eos = max(sorted(counts), key=lambda tok: counts[tok])
    want = [g[: g.index(eos) + 1] if eos in g else g for g in alone]
    assert any(len(w) < new for w in want), "no request ends at the eos: the precondition of this test"
    batch = q4.Batch(a, 3, prefill_rows=4)
    try:
        got = batch.run(requests, new, eos=eos)
        assert got == want
        assert batch.run(requests[:2], 3) == [g[:3] for g in alone[:2]]          # no eos: the token limit alone; the slots were left closed
    finally:
        batch.delete()


def test_run_refuses_bad_arguments_and_closes_its_slots(q4, pairs):
    """ValueError in front of the first open; a pass that raises mid-run (without graphs, a prompt that reaches position 256) leaves no slot open"""
    L = q4.lib()
    a, _ = pairs("pass_long")
    batch = q4.Batch(a, 2, prefill_rows=8)
    try:
        for args, kw in ((([[1, 5]], 0), {}), (([[1, 5]], 4), {"seeds": [1, 2]}), (([[1, 5], []], 4), {}), (([[1] * S], 2), {})):
            with pytest.raises(ValueError):
                batch.run(*args, **kw)
        L.q4_set_use_graphs(0)
        with pytest.raises(q4.Q4Error):
            batch.run([bc.prompt(300, seed=950), bc.prompt(3, seed=951)], 4)
        L.q4_set_use_graphs(1)
        assert batch.pos(0) >= 249 and batch.pos(0) <= 256        # (it ran up to the positions without a row form)
        for slot in range(2):
            assert L.q4_batch_close(batch.h, slot) == ERR_ARG      # not open: run closed what it had opened
        assert len(batch.run([bc.prompt(3, seed=951)], 2)[0]) == 2
    finally:
        L.q4_set_use_graphs(1)
        batch.delete()


# ---- 10. refusals ---------------------------------------------------------------------------------------------------------------------------------------
def test_set_prefill_refuses_other_values(q4, pairs):
    L = q4.lib()
    a, _ = pairs("pass_long")
    batch = q4.Batch(a, 2)
    try:
        assert L.q4_batch_get_prefill(batch.h) == 1
        batch.set_prefill(6)
        for n in (0, 9, -1, 100):
            assert L.q4_batch_set_prefill(batch.h, n) == ERR_ARG and L.q4_batch_get_prefill(batch.h) == 6
        for n in range(1, 9):
            assert L.q4_batch_set_prefill(batch.h, n) == 0 and batch.prefill() == n
    finally:
        batch.delete()
