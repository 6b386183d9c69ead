"""Batched decoding (csrc/q4_batch.hip, the row forms in csrc/prompt_pass.hip): up to eight sequences ("slots") over one Transformer's
weights, one position each per pass over the weights. The invariant every test here holds to: what a slot produces -- its tokens, every K / V row, the
logits of its last position -- is BYTE for byte what the same checkpoint produces when it runs that sequence alone (q4_generate_ids on a second
Transformer of the same file, greedy screen off), whatever the other slots of the pass are doing.

  1. equality: 1, 2, 3, 5 and 8 slots with prompts of 1 .. 40 tokens, 64 passes (24 or more generated tokens per slot);
  2. every attention form in one pass, and bin crossings: slots restored near positions 5, 120, 250, 300 and 2100 and just below every position at which
     the plan of the step's attention changes (tests/pass_context_ref.py restates pass_attention_plan; the boundaries are read from it), each run across
     its boundary, with graphs and without; without graphs the step has no row form at positions 256 .. 510, and a pass with a row there is refused;
  3. the temperature / top-p sampler, another seed per slot;
  4. churn and isolation on poisoned caches: a slot closed mid-run and reopened on another prompt while the others go on;
  5. restore from a snapshot of the model's own sequence, and its refusals;
  6. the model's own sequence is untouched by batch work;
  7. the grouped-query shape; 8. a hostile checkpoint; 9. what q4_batch_new and q4_batch_step refuse (these need a built model, so they live here)."""
import ctypes as C

import numpy as np
import pytest

import batch_cases as bc
import hostile_models as hm
import pass_context_ref as ref
from llama_cu_awq_amd import synth

pytestmark = pytest.mark.gpu

S = 2304                  # pass_long's and gqa7b_pair's context
PASSES = 64               # test 1: prompts of up to 40 tokens, so every slot generates 24 tokens or more
LENGTHS = [1, 3, 8, 9, 17, 30, 37, 40]
CROSS = 20                # test 2: passes per slot, the boundary in the middle
UNSUPPORTED, ERR_ARG = 1, 5


@pytest.fixture(scope="module")
def checkpoints(tmp_path_factory):
    d = tmp_path_factory.mktemp("batch")
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


def _equality(q4, pairs, name, n_slots, lengths):
    a, b = pairs(name)
    batch = q4.Batch(a, n_slots)
    try:
        prompts = [bc.prompt(lengths[i], seed=100 + i) for i in range(n_slots)]
        for i, p in enumerate(prompts):
            batch.open(i, p)
        out = batch.generate(PASSES)
        assert out.shape == (PASSES, q4.BATCH_MAX_SLOTS) and (out[:, n_slots:] == -1).all()
        for i, p in enumerate(prompts):
            bc.assert_slot_equals(q4, batch, i, _alone(q4, b, name, p, PASSES), out, 0, "%s, %d slots, slot %d" % (name, n_slots, i))
    finally:
        batch.delete()


# ---- 1. equality ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_slots", [1, 2, 3, 5, 8])
def test_slots_equal_their_runs_alone(q4, pairs, n_slots):
    _equality(q4, pairs, "pass_long", n_slots, LENGTHS)


def test_step_reports_what_generate_reports(q4, pairs):
    """q4_batch_step pass by pass: -1 inside the prompt, then the run alone's tokens; the position on the device moves by one per pass"""
    a, b = pairs("pass_long")
    p = bc.prompt(3, seed=101)
    solo = _alone(q4, b, "pass_long", p, PASSES)
    batch = q4.Batch(a, 2)
    try:
        batch.open(1, p)
        for i in range(8):
            out = batch.step()
            assert batch.pos(1) == i + 1 and batch.pos(0) == 0
            assert out[1] == (-1 if i + 1 < len(p) else solo.tokens[i + 1]) and (np.delete(out, 1) == -1).all()
    finally:
        batch.delete()


# ---- 2. every attention form in one pass, and bin crossings ---------------------------------------------------------------------------------------------
def _starts(mode):
    """Where test 2's slots start: the issue's positions, and CROSS / 2 below every position at which the plan of the step's attention changes (the form,
    the chunk size or -- with bins -- the bin argument, which sets the chunk count); where no row form exists below a boundary (no graphs: 256 .. 510),
    the boundary itself. Kept: the starts whose CROSS positions all have a form."""
    def plan(pos):
        return ref.form(pos, mode, S), (ref.bin_arg(pos, mode, S) if mode else 0)
    edges = [pos for pos in range(1, S - CROSS) if plan(pos) != plan(pos - 1)]
    starts = [5, 120, 250, 300, 2100] + [e - CROSS // 2 for e in edges] + [e for e in edges if ref.form(e - 1, mode, S) is None]
    return edges, sorted({s for s in starts if all(ref.form(s + i, mode, S) is not None for i in range(CROSS))})


@pytest.mark.parametrize("mode", [1, 0])
def test_every_attention_form_in_one_pass(q4, pairs, mode):
    L = q4.lib()
    a, b = pairs("pass_long")
    edges, starts = _starts(mode)
    if mode:
        assert edges == [128, 256, 512, 1024, 2048] and len(starts) == 10, (edges, starts)      # (what the plan gives at this context: every one is crossed)
    else:
        assert {ref.form(s + i, mode, S) for s in starts for i in range(CROSS)} == {"v", 64, 128, 256}, starts
    long_prompt = bc.prompt(S, seed=200)
    L.q4_set_use_graphs(mode)
    snaps = []
    try:
        # every slot runs the same long sequence from its own start: the run alone gives the reference AND, through a snapshot of its first rows, the prefix
        runs = []
        for s in starts:
            solo = bc.Solo(q4, b, long_prompt[: s + 1], s + CROSS, first_row=s)
            snaps.append(b.snapshot(s))
            runs.append(solo)
        for first in range(0, len(starts), q4.BATCH_MAX_SLOTS):
            group = list(range(first, min(first + q4.BATCH_MAX_SLOTS, len(starts))))
            if len(group) == 1 and first > 0:       # (a lone row is test 1's case: keep it among others)
                group = [first - 1] + group
            batch = q4.Batch(a, len(group))
            try:
                for slot, g in enumerate(group):
                    batch.restore(slot, snaps[g], long_prompt[: starts[g] + 1])
                out = batch.generate(CROSS)
                assert out.shape[0] == CROSS
                for slot, g in enumerate(group):
                    bc.assert_slot_equals(q4, batch, slot, runs[g], out, starts[g], "graphs %d, start %d" % (mode, starts[g]))
            finally:
                batch.delete()
    finally:
        for s in snaps:
            s.close()
        L.q4_set_use_graphs(1)


def test_a_row_without_a_row_form_is_refused(q4, pairs):
    """without graphs the step at positions 256 .. 510 runs the one-block form, which no pass restates: the pass is refused and nothing moves"""
    L = q4.lib()
    a, b = pairs("pass_long")
    assert ref.form(300, 0, S) is None
    p = bc.prompt(302, seed=201)
    b.generate_ids(p, 301)
    snap = b.snapshot(300)
    batch = q4.Batch(a, 2)
    try:
        batch.open(0, bc.prompt(4, seed=202))
        batch.restore(1, snap, p)
        L.q4_set_use_graphs(0)
        out = np.zeros(q4.BATCH_MAX_SLOTS, dtype=np.int32)
        assert L.q4_batch_step(batch.h, a.sampler, out.ctypes.data) == UNSUPPORTED
        assert batch.pos(0) == 0 and batch.pos(1) == 300
        L.q4_set_use_graphs(1)
        assert batch.step()[1] == -1 and batch.pos(0) == 1 and batch.pos(1) == 301
    finally:
        L.q4_set_use_graphs(1)
        batch.delete()
        snap.close()


# ---- 3. the temperature / top-p sampler ----------------------------------------------------------------------------------------------------------------
def test_sampled_slots_equal_their_runs_alone(q4, pairs):
    a, b = pairs("pass_long")
    seeds = [11, 12, 13, 14, 15]
    prompts = [bc.prompt(LENGTHS[i], seed=300 + i) for i in range(len(seeds))]
    try:
        runs = []
        for p, seed in zip(prompts, seeds):
            bc.set_sampler(q4, b, 0.5, 0.6, seed)
            runs.append(bc.Solo(q4, b, p, PASSES))
        bc.set_sampler(q4, a, 0.5, 0.6, 999)        # (its own stream is not used: a slot's coins come from the slot's seed)
        batch = q4.Batch(a, len(seeds))
        try:
            for i, (p, seed) in enumerate(zip(prompts, seeds)):
                batch.open(i, p, seed=seed)
            out = batch.generate(PASSES)
            for i, solo in enumerate(runs):
                bc.assert_slot_equals(q4, batch, i, solo, out, 0, "sampled, slot %d (seed %d)" % (i, seeds[i]))
            assert len({tuple(r.tokens[len(r.prompt):len(r.prompt) + 8]) for r in runs}) > 1     # (the seeds matter)
        finally:
            batch.delete()
    finally:
        bc.set_sampler(q4, a, 0.0, 0.9, 1)
        bc.set_sampler(q4, b, 0.0, 0.9, 1)


# ---- 4. churn and isolation ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", ["nan", "huge"])
def test_churn_on_poisoned_caches(q4, pairs, pattern):
    a, b = pairs("pass_long")
    first, second = 12, 14
    prompts = [bc.prompt(n, seed=400 + n) for n in (5, 9, 2)]
    newcomer = bc.prompt(6, seed=444)
    batch = q4.Batch(a, 3)
    try:
        for slot in range(3):
            bc.poison_slot(q4, batch, slot, pattern)
        for slot, p in enumerate(prompts):
            batch.open(slot, p)
        out1 = batch.generate(first)
        kept = bc.slot_rows(q4, batch, 1, 0, first)
        batch.close(1)
        batch.open(1, newcomer)
        out2 = batch.generate(second)
        out = np.concatenate([out1, out2])
        total = first + second
        for slot in (0, 2):
            bc.assert_slot_equals(q4, batch, slot, _alone(q4, b, "pass_long", prompts[slot], total), out, 0, "%s, survivor %d" % (pattern, slot))
            bc.assert_poison_above(q4, batch, slot, total, pattern, "%s, survivor %d" % (pattern, slot))
        bc.assert_slot_equals(q4, batch, 1, _alone(q4, b, "pass_long", newcomer, second), out, 0, "%s, newcomer" % pattern, first_pass=first)
        bc.assert_poison_above(q4, batch, 1, second, pattern, "%s, newcomer" % pattern)      # (it ran further than the sequence it replaced)
        closed = _alone(q4, b, "pass_long", prompts[1], first)
        assert np.array_equal(kept[0], closed.k) and np.array_equal(kept[1], closed.v), "%s: the closed slot's rows" % pattern
    finally:
        batch.delete()


# ---- 5. restore ----------------------------------------------------------------------------------------------------------------------------------------
def test_restore_behind_an_ingested_prefix(q4, pairs):
    L = q4.lib()
    a, b = pairs("pass_long")
    p = bc.prompt(60, seed=500)
    steps, n_pos = 60 + bc.GEN, 41
    solo = _alone(q4, b, "pass_long", p, steps)
    a.generate_ids(p, 50)                       # the prefix comes from the batch's own model: prompt passes on its own sequence
    snap = a.snapshot(n_pos)
    batch = q4.Batch(a, 2)
    try:
        assert L.q4_batch_restore(batch.h, 0, snap.h, np.asarray(p[:n_pos], dtype=np.int32).ctypes.data, n_pos, 1) == ERR_ARG      # no pending token
        wrong = np.asarray(p, dtype=np.int32)
        wrong[7] += 1
        assert L.q4_batch_restore(batch.h, 0, snap.h, wrong.ctypes.data, len(p), 1) == ERR_ARG
        assert L.q4_batch_restore(batch.h, 0, None, wrong.ctypes.data, len(p), 1) == ERR_ARG
        batch.restore(0, snap, p)
        assert batch.pos(0) == n_pos
        out = batch.generate(steps - n_pos)
        bc.assert_slot_equals(q4, batch, 0, solo, out, n_pos, "restored at %d" % n_pos)
    finally:
        batch.delete()
        snap.close()


# ---- 6. the model's own sequence ------------------------------------------------------------------------------------------------------------------------
def test_the_models_own_sequence_is_untouched(q4, pairs):
    import cache_poison as cp
    a, b = pairs("pass_long")
    p = bc.prompt(10, seed=600)
    solo = _alone(q4, b, "pass_long", p, 48)
    half = a.generate_ids(p, 24)[0].copy()
    assert np.array_equal(half, solo.tokens[:25])
    batch = q4.Batch(a, 3)
    try:
        for slot in range(3):
            batch.open(slot, bc.prompt(4 + slot, seed=610 + slot))
        batch.generate(30)
        assert a.pos() == 24 and a.common_prefix(half) == 24
        toks = a.generate_ids(half, 48, reuse=True)[0]
        assert np.array_equal(toks, solo.tokens)
        k, v = cp.read_rows(q4, a, 0, 48)
        assert np.array_equal(k, solo.k) and np.array_equal(v, solo.v)
        assert np.array_equal(a.logits().view(np.uint16), solo.logits)
    finally:
        batch.delete()


# ---- 7. grouped-query, 8. hostile weights ---------------------------------------------------------------------------------------------------------------
def test_grouped_query_slots_equal_their_runs_alone(q4, pairs):
    _equality(q4, pairs, "gqa7b_pair", 3, [2, 11, 33])


def test_hostile_weights(q4, pairs):
    _equality(q4, pairs, "pass_long/combined", 3, [4, 19, 40])


# ---- 9. refusals ----------------------------------------------------------------------------------------------------------------------------------------
def test_arguments_are_refused(q4, pairs):
    L = q4.lib()
    a, _ = pairs("pass_long")
    h = C.c_void_p()
    for n in (0, 9, -1):
        assert L.q4_batch_new(C.byref(h), a.h, n) == ERR_ARG
    assert L.q4_batch_new(None, a.h, 2) == ERR_ARG and q4.Batch.covers(a)
    batch = q4.Batch(a, 2)
    try:
        good = np.asarray([1, 5, 6], dtype=np.int32)
        out = np.zeros(q4.BATCH_MAX_SLOTS, dtype=np.int32)
        for slot in (-1, 2, 8):
            assert L.q4_batch_open(batch.h, slot, good.ctypes.data, 3, 1) == ERR_ARG and L.q4_batch_close(batch.h, slot) == ERR_ARG
            assert L.q4_batch_pos(batch.h, slot) == -ERR_ARG and L.q4_batch_get_logits(batch.h, slot, out.ctypes.data) == ERR_ARG
        assert L.q4_batch_open(batch.h, 0, good.ctypes.data, 0, 1) == ERR_ARG and L.q4_batch_open(batch.h, 0, None, 3, 1) == ERR_ARG
        assert L.q4_batch_open(batch.h, 0, good.ctypes.data, S + 1, 1) == ERR_ARG
        for bad in ([1, 512, 6], [1, -1, 6]):
            assert L.q4_batch_open(batch.h, 0, np.asarray(bad, dtype=np.int32).ctypes.data, 3, 1) == ERR_ARG
        assert L.q4_batch_close(batch.h, 0) == ERR_ARG                                   # not open
        assert (batch.step() == -1).all()                                                # no open slot: nothing runs
        batch.open(0, good)
        assert L.q4_batch_open(batch.h, 0, good.ctypes.data, 3, 1) == ERR_ARG            # already open
        assert L.q4_batch_step(batch.h, None, out.ctypes.data) == ERR_ARG and L.q4_batch_step(batch.h, a.sampler, None) == ERR_ARG
        assert L.q4_batch_get_kv_row(batch.h, 0, 2, 0, out.ctypes.data, out.ctypes.data) == ERR_ARG
        assert L.q4_batch_get_kv_row(batch.h, 0, 0, S, out.ctypes.data, out.ctypes.data) == ERR_ARG
        assert batch.pos(0) == 0
        # a sampler with a logit stage on, or log-probability records switched on behind q4_batch_new: the pass is refused, nothing moves (a guide: the next test)
        a.set_sampling(top_k=5)
        assert L.q4_batch_step(batch.h, a.sampler, out.ctypes.data) == UNSUPPORTED
        a.set_sampling()
        a.set_logprobs(0)
        assert L.q4_batch_step(batch.h, a.sampler, out.ctypes.data) == UNSUPPORTED and not q4.Batch.covers(a)
        assert L.q4_batch_new(C.byref(h), a.h, 2) == UNSUPPORTED
        a.set_logprobs(None)
        assert batch.pos(0) == 0 and batch.step()[0] == -1 and batch.pos(0) == 1
    finally:
        a.set_sampling()
        a.set_logprobs(None)
        batch.delete()


def test_settings_that_are_not_admitted(q4, pairs):
    """A guide on the model, a fusion level below 3, a temperature the row sampler does not take: q4_batch_covers / q4_batch_new refuse the guide, and a
    step of a batch built before refuses each with the unsupported status, nothing launched: the positions do not move, and the batch goes on afterwards"""
    L = q4.lib()
    a, b = pairs("pass_long")
    p = bc.prompt(3, seed=900)
    solo = _alone(q4, b, "pass_long", p, PASSES)
    out = np.zeros(q4.BATCH_MAX_SLOTS, dtype=np.int32)
    h = C.c_void_p()
    guide = q4.Guide(np.zeros((1, a.config.vocab_size), dtype=np.uint16))      # one state, every token allowed
    batch = q4.Batch(a, 2)
    try:
        batch.open(0, p)
        batch.open(1, bc.prompt(5, seed=901))
        assert batch.step()[0] == -1

        def refused(what):
            assert L.q4_batch_step(batch.h, a.sampler, out.ctypes.data) == UNSUPPORTED, what
            n = C.c_int(-1)
            assert L.q4_batch_generate(batch.h, a.sampler, 2, out.ctypes.data, C.byref(n)) == UNSUPPORTED and n.value == -1, what
            assert batch.pos(0) == 1 and batch.pos(1) == 1, what

        a.set_guide(guide)
        assert not q4.Batch.covers(a) and L.q4_batch_new(C.byref(h), a.h, 2) == UNSUPPORTED and not h.value
        refused("a guide")
        a.set_guide(None)
        assert q4.Batch.covers(a)
        L.q4_set_fusion(2)
        refused("fusion level 2")
        L.q4_set_fusion(q4.DEFAULT_FUSION)
        bc.set_sampler(q4, a, -0.5, 0.6, 1)
        refused("a negative temperature")
        bc.set_sampler(q4, a, 0.0, 0.9, 1)
        toks = batch.generate(6)
        assert [int(x) for x in toks[1:, 0]] == [int(x) for x in solo.tokens[3:8]] and batch.pos(0) == 7
    finally:
        a.set_guide(None)
        L.q4_set_fusion(q4.DEFAULT_FUSION)
        bc.set_sampler(q4, a, 0.0, 0.9, 1)
        batch.delete()
        guide.close()


@pytest.mark.parametrize("name,kv", [("head128_k5120", "fp16"), ("tinyllama", "fp16"), ("k5120_pair", "fp16"), ("pass_long", "fp8")])
def test_shapes_that_are_not_admitted(q4, checkpoints, name, kv):
    """13B-wide shapes, another width or head size, the FP8 cache: q4_batch_covers is 0 and q4_batch_new refuses with the unsupported status"""
    L = q4.lib()
    t = q4.Transformer(checkpoints(name), kv=kv, pass_13b=True, pass_kv8=True, pass_gqa=True)
    try:
        h = C.c_void_p()
        assert not q4.Batch.covers(t) and L.q4_batch_new(C.byref(h), t.h, 2) == UNSUPPORTED and not h.value
    finally:
        t.close()
