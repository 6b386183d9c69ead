"""DRY and the no-repeat-n-gram ban inside the decode step (csrc/q4_dry.hip, q4_sampler_set_dry / _set_dry_breakers, q4_dry_penalty): the launch on
crafted rings against the numpy reference (tests/dry_ref.py) BIT FOR BIT, and the launch inside the step in every graph form against a ground truth
rebuilt from a DRY-off model's raw logits."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import dry_ref as ref
import sampling_controls_ref as sc_ref
from conftest import GOLDEN, ROOT
from llama_cu_awq_amd import synth

pytestmark = pytest.mark.gpu

ERR_ARG = 5
DRY = dict(multiplier=0.8, base=1.75, allowed_length=2, last_n=1024, no_repeat_ngram_size=0)
# per mode, inside the step: a sampled run at 0.8 / 0.9 seldom repeats a 2-gram of its own (DRY at allowed_length 2 touched an entry in ONE of its 298
# generating steps), so it runs with allowed_length 1 -- every token that returns is a match -- to keep the comparison from passing vacuously
DRY_FOR = {"greedy": DRY, "sampled": dict(DRY, allowed_length=1)}
BAN = dict(multiplier=0.0, base=1.75, allowed_length=2, last_n=1024, no_repeat_ngram_size=4)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float16).view(np.uint16)


def _pen(q4, c):
    return q4.dry_penalty_table(multiplier=c["multiplier"], base=c["base"], allowed_length=c["allowed_length"])


def _want(q4, x, ring, pos, c, breakers=()):
    return ref.apply(x, ring, pos, _pen(q4, c), breakers=breakers, **c)


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. the op against the reference
HIGH = 65536


def _cases(n):
    """(name, ring, pos, controls, breakers, logits, must_touch) -- every ring holds a few entries behind pos, which the launch must not read into the
    window. Token z = 0 is in range for every n; `b` and `c` are in range where the vocabulary has them and plain ints outside it elsewhere. A vocabulary
    beyond 16 bits of token id (n > 65536) runs the same cases on z, b, c = 100003, 70001, 128255: every ring token in range, every breaker and every
    touched entry then has an id >= 65536."""
    rng = np.random.default_rng(7000 + n)
    z = 100003 if n > HIGH else 0
    b, c, X = (70001, 128255, n + 5) if z else ((1 if n >= 2 else n + 9), (2 if n >= 3 else n + 11), n + 5)
    length = 5004

    def periodic(vals):
        return np.tile(np.array(vals, dtype=np.int64), length // len(vals) + 1)[:length].astype(np.int32)

    per3, one = periodic([z, b, c]), np.full(length, z, dtype=np.int32)   # per3[p] == c and the next token is z wherever p % 3 == 2
    a2 = rng.integers(0, 2, length).astype(np.int32)
    if n < 2 or z:
        a2 = np.where(a2 == 1, b, z).astype(np.int32)
    out = []

    def add(name, ring, pos, breakers=(), touch=True, x=None, **over):
        ctl = dict(DRY)
        ctl.update(over)
        out.append((name, ring, pos, ctl, list(breakers), (rng.standard_normal(n) * 3.0).astype(np.float16) if x is None else x, touch))

    # windows: p = 0; p < last_n; last_n 1, 2, 64, 1024, 4096 with p up to 5000. A window of ONE entry (p = 0, last_n = 1) has no index in [start, p):
    # the rule can touch nothing there, whatever the ring
    add("p = 0", one, 0, allowed_length=1, touch=False)
    add("last_n 1", one, 100, last_n=1, allowed_length=1, touch=False)
    add("p < last_n", per3, 11, last_n=64)
    add("last_n 2", one, 100, last_n=2, allowed_length=1)
    add("last_n 64, period 3", per3, 200, last_n=64)
    add("last_n 1024, period 3", per3, 1499)
    add("last_n 4096, period 3", per3, 5000, last_n=4096)
    add("last_n 1024, one token", one, 1500)
    add("last_n 4096, one token: the worst case", one, 5000, last_n=4096)
    add("last_n 64, alphabet 2", a2, 300, last_n=64)
    add("last_n 4096, alphabet 2", a2, 5000, last_n=4096)
    add("alphabet 2, ban 3 and DRY", a2, 301, last_n=64, no_repeat_ngram_size=3)
    # ids outside [0, n): as the last token, inside a match, as the next token (one flaw makes one candidate's next token valid)
    add("outside: the last token", periodic([z, b, X]), 200)
    add("outside: inside the match", periodic([z, X, b]), 200)
    flawed = periodic([z, b, X])
    flawed[8] = z
    add("outside: the next token", flawed, 199)
    add("outside: huge ids", periodic([z, 2 ** 31 - 1, -2 ** 31]), 200)
    # breakers: the last token itself; at distance 1, 2 and 64 (a token of its own in a ring of zeros: R is exactly the distance; a vocabulary of one
    # token has no second id that could be that breaker)
    add("breaker at p", one, 1500, breakers=[z], touch=False)
    if n >= 2:
        many = list(range(z + 1, min(n, z + 700)))
        for d, allowed, ids in ((1, 1, [b]), (2, 2, many), (64, 5, [b])):
            ring = one.copy()
            ring[1500 - d] = ids[-1]
            add("breaker at distance %d" % d, ring, 1500, breakers=ids, allowed_length=allowed)
            if d < 64:
                add("breaker at distance %d, allowed one more" % d, ring, 1500, breakers=ids, allowed_length=d + 1, touch=False)
    # allowed_length x base (4.0 reaches the clamp at -65504: M = 64)
    for allowed in (1, 2, 5):
        for base in (1.0, 1.75, 4.0):
            add("allowed %d base %g" % (allowed, base), per3, 1499, allowed_length=allowed, base=base)
    # the ban, with and without DRY (65 needs M = 64)
    for ngram in (0, 2, 3, 65):
        for multiplier in (0.0, 0.8):
            add("ngram %d multiplier %g" % (ngram, multiplier), per3, 1499, no_repeat_ngram_size=ngram, multiplier=multiplier,
                touch=bool(ngram or multiplier))
    add("ngram 65, a match of 62", per3[4936:], 64, no_repeat_ngram_size=65, multiplier=0.0, touch=False)
    # touched logits among -inf, +inf, NaN, +-65504, -0 (the touched token of per3 at p % 3 == 2 is z)
    for v in (-np.inf, np.inf, np.nan, 65504.0, -65504.0, -0.0):
        x = (rng.standard_normal(n) * 3.0).astype(np.float16)
        x[z] = v
        add("touched %r" % v, per3, 1499, x=x)
        add("touched %r, base 4" % v, per3, 1499, x=x, base=4.0)
        add("banned %r" % v, per3, 1499, x=x, no_repeat_ngram_size=2)
    return out


def _apply(q4, dl, x, dr, dp, ctl, breakers):
    dl.put(x)
    q4.dry_penalty(dl, x.shape[0], breakers=breakers, tokens=dr, pos=dp, **ctl)
    q4.synchronize()
    return dl.get(np.float16, x.shape[0])


@pytest.mark.parametrize("n", [1, 8, 1027, 32000, 40000, 128256, 128259])
def test_op_matches_the_reference_bit_for_bit(q4, n):
    dl, dp = q4.DevBuf(nbytes=2 * n), q4.DevBuf(nbytes=4)
    rings = {}
    touched_cases = highest = 0
    for name, ring, pos, ctl, breakers, x, must_touch in _cases(n):
        what = "n %d, %s" % (n, name)
        if id(ring) not in rings:
            rings[id(ring)] = (ring, q4.DevBuf(ring))              # (the array is kept: its id must not be reused)
        dp.put(np.array([pos], dtype=np.int32))
        got = _apply(q4, dl, x, rings[id(ring)][1], dp, ctl, breakers)
        want, touched = _want(q4, x, ring, pos, ctl, breakers)
        bad = np.nonzero(_bits(got) != _bits(want))[0]
        assert bad.size == 0, "%s: %d entries differ, first %d: got %04x, reference %04x (input %04x)" % (
            what, bad.size, bad[0], _bits(got)[bad[0]], _bits(want)[bad[0]], _bits(x)[bad[0]])
        untouched = np.setdiff1d(np.arange(n), touched)
        assert _bits(got)[untouched].tobytes() == _bits(x)[untouched].tobytes(), what + ": an untouched entry changed"
        assert bool(touched) == must_touch, "%s: the reference touched %s" % (what, touched)
        if n > HIGH:                                                   # beyond 16 bits of id: what the reference touches, the breakers, the ring's ids in range
            assert all(t >= HIGH for t in touched) and all(t >= HIGH for t in breakers), (what, touched)
            assert ((ring >= HIGH) | (ring < 0) | (ring >= n)).all(), what
            highest = max([highest] + [int(t) for t in touched])
        again = _apply(q4, dl, x, rings[id(ring)][1], dp, ctl, breakers)
        assert again.tobytes() == got.tobytes(), what + ": a second launch gave other bytes"
        touched_cases += bool(touched)
    assert touched_cases >= 40
    assert n <= HIGH or highest > 98304, highest


def test_op_argument_errors_leave_the_logits_alone(q4):
    L = q4.lib()
    n = 1000
    x = (np.random.default_rng(6).standard_normal(n) * 2.0).astype(np.float16)
    ring = np.zeros(64, dtype=np.int32)
    dl, dr, dp = q4.DevBuf(x), q4.DevBuf(ring), q4.DevBuf(np.array([40], dtype=np.int32))
    ids = np.array([3, n], dtype=np.int32)
    for kw, brk in ((dict(last_n=4097), 0), (dict(no_repeat_ngram_size=1), 0), (dict(base=0.5), 0), (dict(), 2)):
        c = q4.DryControls(**dict(DRY, **kw))
        assert L.q4_dry_penalty(dl.ptr, n, C.byref(c), ids.ctypes.data if brk else None, brk, dr.ptr, dp.ptr) == ERR_ARG, (kw, brk)
        q4.synchronize()
        assert dl.get(np.float16, n).tobytes() == x.tobytes(), (kw, brk)
    q4.dry_penalty(dl, n, breakers=[3], tokens=dr, pos=dp, **DRY)      # ... and the same call with valid arguments does rewrite
    q4.synchronize()
    assert dl.get(np.float16, n).tobytes() == _want(q4, x, ring, 40, DRY, [3])[0].tobytes() != x.tobytes()


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. inside the step
PROMPT = [1, 5, 9]
V40K_PROMPT = [1, 5, 9, 5, 9, 5]                                 # a repetition in the prompt: 32 steps of a random model need not produce one
SAMPLED = (0.8, 0.9)
SEED = 4242
STEPS = 300                                                      # small: the bins 128 / 256, eight steps per replay
CONTROLS = dict(top_k=40, repeat_penalty=1.3, penalty_last_n=16)


def _sampler(mode):
    return dict(temperature=SAMPLED[0], topp=SAMPLED[1], seed=SEED) if mode == "sampled" else dict(temperature=0.0)


@pytest.fixture(scope="module")
def paths(tmp_path_factory):
    d = tmp_path_factory.mktemp("dry")
    out = {}
    for name in ("small", "v40k"):
        out[name] = str(d / (name + ".bin"))
        synth.write_model(out[name], name, seed=7)
    return out


def _stepwise(q4, t, prompt, steps):
    """the reference-shaped loop: one run_transformer call per step, synchronised, the next token read from the ring by the device"""
    t.reset(prompt)
    for pos in range(steps):
        t.run_transformer(pos >= len(prompt) - 1)
        q4.synchronize()
    return np.array([t.token(i) for i in range(steps + 1)], dtype=np.int32)


def _raw_logits(q4, path, tokens):
    """the sequence teacher-forced through a model WITHOUT DRY, one graph replay per step: the raw fp16 logits of every position"""
    t = q4.Transformer(path)
    t.reset(tokens)
    out = []
    for pos in range(len(tokens) - 1):
        t.run_transformer_at(pos, 0)
        out.append(t.logits())
    t.close()
    return np.stack(out)


def _predict(q4, orc, raw, tokens, n_prompt, dry, mode, breakers=(), controls=None):
    """what every generating step must have chosen: DRY over the raw logits and the ring, then the sampling controls' reference, then the argmax (lowest
    index) or the restated sampler with the seed's coin stream (one coin per step, prompt steps included). Returns (ring, processed logits of the last
    step, generating steps in which DRY touched an entry)."""
    L = q4.lib()
    state = C.c_ulonglong(SEED)
    pen = _pen(q4, dry)
    out = np.array(tokens, dtype=np.int32).copy()
    touched_steps, x = 0, None
    for p in range(len(tokens) - 1):
        coin = L.random_f32(C.byref(state))
        if p < n_prompt - 1:
            continue
        x, touched = ref.apply(raw[p], tokens, p, pen, breakers=breakers, **dry)
        touched_steps += bool(touched)
        if controls:
            x = sc_ref.process(x, tokens=tokens, pos=p, **controls)
        if mode == "greedy":
            out[p + 1] = int(np.argmax(x.astype(np.float32)))
        else:
            out[p + 1] = orc.lib().orc_sample_topp(orc.f16_bits(x.copy()), x.shape[0], SAMPLED[0], SAMPLED[1], coin)
    return out, x, touched_steps


def _repeated(tokens, k):
    grams = [tuple(tokens[i:i + k]) for i in range(len(tokens) - k + 1)]
    return len(grams) - len(set(grams))


@pytest.fixture(scope="module")
def runs(q4, paths):
    """per mode, once: the run that never called a setter, the DRY run (eight steps per replay), the DRY stepwise run, the raw logits of the DRY run's
    ring, the run under the 4-gram ban"""
    L = q4.lib()
    out = {}
    for mode in ("greedy", "sampled"):
        c0 = L.q4_graph_captures()
        t = q4.Transformer(paths["small"], **_sampler(mode))
        plain = t.generate_ids(PROMPT, STEPS)[0].copy()
        r = dict(plain=plain, plain_logits=t.logits(), plain_captures=L.q4_graph_captures() - c0)
        t.close()
        t = q4.Transformer(paths["small"], dry=DRY_FOR[mode], **_sampler(mode))
        r["tokens"] = t.generate_ids(PROMPT, STEPS)[0].copy()
        r["logits"] = t.logits()
        t.close()
        t = q4.Transformer(paths["small"], dry=DRY_FOR[mode], **_sampler(mode))
        r["stepwise"] = _stepwise(q4, t, PROMPT, STEPS)
        t.close()
        t = q4.Transformer(paths["small"], dry=BAN, **_sampler(mode))
        r["banned"] = t.generate_ids(PROMPT, STEPS)[0].copy()
        t.close()
        r["raw"] = _raw_logits(q4, paths["small"], r["tokens"]) if len(r["tokens"]) == STEPS + 1 else None
        out[mode] = r
    return out


@pytest.mark.parametrize("mode", ["greedy", "sampled"])
def test_grouped_steps_equal_the_stepwise_loop(runs, mode):
    """(a) generate_ids (eight steps per replay, the bins 128 / 256) against one run_transformer call per step"""
    r = runs[mode]
    assert len(r["tokens"]) == STEPS + 1, "the run stopped at an EOS: pick another seed"
    assert np.array_equal(r["tokens"], r["stepwise"]), "first difference at %d" % int(np.nonzero(r["tokens"] != r["stepwise"])[0][0])


@pytest.mark.parametrize("mode", ["greedy", "sampled"])
def test_tokens_are_what_the_reference_predicts(q4, orc, runs, mode):
    """(b) the DRY run's ring, rebuilt from a DRY-off model's raw logits, the numpy reference and the argmax / the restated sampler; (d) the inputs
    are not vacuous: the plain greedy run loops, DRY changes it, the reference touched an entry in at least 10 generating steps"""
    r = runs[mode]
    want, last, touched_steps = _predict(q4, orc, r["raw"], r["tokens"], len(PROMPT), DRY_FOR[mode], mode)
    bad = np.nonzero(want != r["tokens"])[0]
    assert bad.size == 0, "%s: %d tokens differ, first at ring index %d: %d, reference %d" % (mode, bad.size, bad[0], r["tokens"][bad[0]], want[bad[0]])
    print("%s: DRY touched an entry in %d generating steps; %d distinct tokens (plain %d), repeated 8-grams %d (plain %d)" % (
        mode, touched_steps, len(set(r["tokens"].tolist())), len(set(r["plain"].tolist())), _repeated(r["tokens"].tolist(), 8),
        _repeated(r["plain"].tolist(), 8)))
    assert touched_steps >= 10, touched_steps
    assert not np.array_equal(r["tokens"], r["plain"]), "DRY changed nothing"
    if mode == "greedy":
        assert _repeated(r["plain"].tolist(), 8) >= 50, "the plain greedy run does not loop: pick another prompt"
        assert r["logits"].tobytes() == last.tobytes()           # after a greedy generating step RunState::logits holds the PROCESSED logits


@pytest.mark.parametrize("mode", ["greedy", "sampled"])
def test_no_4_gram_occurs_twice_under_the_ban(runs, mode):
    """(c) no_repeat_ngram_size = 4, multiplier 0, last_n = 1024: an exact invariant of the ring, no reference needed"""
    r = runs[mode]
    assert len(r["banned"]) == STEPS + 1, "the run stopped at an EOS: pick another seed"
    assert _repeated(r["banned"].tolist(), 4) == 0
    if mode == "greedy":
        assert _repeated(r["plain"].tolist(), 4) > 0 and not np.array_equal(r["banned"], r["plain"])


def test_large_vocabulary_greedy(q4, orc, paths):
    """(a), (b) on a vocabulary of 40000 (above the register paths of the neighbouring launches), its whole context, allowed_length 1 and breakers"""
    dry, steps, breakers = dict(DRY, allowed_length=1, last_n=16), 32, [9, 39999]
    t = q4.Transformer(paths["v40k"], dry=dry, dry_breakers=breakers)
    tokens = t.generate_ids(V40K_PROMPT, steps)[0].copy()
    logits = t.logits()
    stepwise = _stepwise(q4, t, V40K_PROMPT, steps)
    t.close()
    assert len(tokens) == steps + 1 and np.array_equal(tokens, stepwise)
    raw = _raw_logits(q4, paths["v40k"], tokens)
    want, last, touched_steps = _predict(q4, orc, raw, tokens, len(V40K_PROMPT), dry, "greedy", breakers=breakers)
    assert np.array_equal(want, tokens) and logits.tobytes() == last.tobytes()
    assert touched_steps >= 1


@pytest.mark.parametrize("mode", ["greedy", "sampled"])
def test_dry_composes_with_the_sampling_controls(q4, orc, paths, runs, mode):
    """(e) DRY with top-k 40 and a repetition penalty: DRY first, then the controls"""
    steps = 120
    t = q4.Transformer(paths["small"], dry=DRY_FOR[mode], sampling=CONTROLS, **_sampler(mode))
    tokens = t.generate_ids(PROMPT, steps)[0].copy()
    logits = t.logits()
    t.close()
    assert len(tokens) == steps + 1
    raw = _raw_logits(q4, paths["small"], tokens)
    want, last, touched_steps = _predict(q4, orc, raw, tokens, len(PROMPT), DRY_FOR[mode], mode, controls=CONTROLS)
    assert np.array_equal(want, tokens), "first difference at %d" % int(np.nonzero(want != tokens)[0][0])
    assert touched_steps >= 1
    if mode == "greedy":
        assert logits.tobytes() == last.tobytes()
        assert (~np.isneginf(logits)).sum() == CONTROLS["top_k"]      # top-k counted what DRY left


def test_a_guides_ban_stays_a_ban(q4, orc, paths, runs):
    """(f) a one-state guide that forbids a token: the launch order is guide, DRY -- the processed logits are DRY over the masked raw logits, the
    forbidden token stays -inf and never appears"""
    steps = 100
    banned = int(runs["greedy"]["tokens"][len(PROMPT)])
    table = np.zeros((1, 1024), dtype=np.uint16)
    table[0, banned] = q4.GUIDE_DEAD
    g = q4.Guide(table)
    t = q4.Transformer(paths["small"], dry=DRY, guide=g)
    tokens = t.generate_ids(PROMPT, steps)[0].copy()
    logits = t.logits()
    t.close()
    g.close()
    assert len(tokens) == steps + 1 and banned not in tokens[len(PROMPT):].tolist()
    raw = _raw_logits(q4, paths["small"], tokens)
    raw[:, banned] = -np.inf                                     # the guide's mask in front of DRY
    want, last, touched_steps = _predict(q4, orc, raw, tokens, len(PROMPT), DRY, "greedy")
    assert np.array_equal(want, tokens) and touched_steps >= 1
    assert logits.tobytes() == last.tobytes() and np.isneginf(logits[banned])


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. off is exactly today
@pytest.mark.parametrize("mode", ["greedy", "sampled"])
def test_off_is_exactly_today(q4, paths, runs, mode):
    """DRY set and cleared again, or set to values that mean off: tokens, the final logits' bytes and the graphs captured are those of a run that
    never called a setter"""
    L = q4.lib()
    r = runs[mode]
    for how in ("cleared", "multiplier 0", "last_n 0"):
        c0 = L.q4_graph_captures()
        t = q4.Transformer(paths["small"], **_sampler(mode))
        if how == "cleared":
            t.set_dry(**DRY)
            t.set_dry_breakers([5, 9])
            t.set_dry()
            t.set_dry_breakers(None)
        elif how == "multiplier 0":
            t.set_dry(multiplier=0.0, base=2.0, allowed_length=3, last_n=64, no_repeat_ngram_size=0)
            t.set_dry_breakers([5, 9])
        else:
            t.set_dry(**dict(DRY, last_n=0, no_repeat_ngram_size=3))
        toks = t.generate_ids(PROMPT, STEPS)[0].copy()
        logits = t.logits()
        t.close()
        assert np.array_equal(toks, r["plain"]), how
        assert logits.tobytes() == r["plain_logits"].tobytes(), how
        assert L.q4_graph_captures() - c0 == r["plain_captures"], how


def test_changing_a_value_between_generations_captures_nothing(q4, orc, paths, runs):
    """the values are not part of a graph: another multiplier, other breakers and the ban for the second generation on ONE model -- the second ring is
    what the reference predicts for the new values and no graph is captured again; a breaker id beyond the vocabulary is found by the first step"""
    L = q4.lib()
    r = runs["greedy"]
    steps = 80
    t = q4.Transformer(paths["small"], dry=DRY)
    first = t.generate_ids(PROMPT, steps)[0].copy()
    assert np.array_equal(first, r["tokens"][:steps + 1])
    c0 = L.q4_graph_captures()
    second_dry, breakers = dict(DRY, multiplier=3.0, allowed_length=1, no_repeat_ngram_size=3), sorted({int(first[60]), 1023})
    t.set_dry(**second_dry)
    t.set_dry_breakers(breakers)
    assert t.dry() == q4.DryControls(**second_dry).as_dict()
    second = t.generate_ids(PROMPT, steps)[0].copy()
    assert L.q4_graph_captures() == c0, "changing a value captured graphs again"
    assert not np.array_equal(second, first)
    want, _, touched_steps = _predict(q4, orc, _raw_logits(q4, paths["small"], second), second, len(PROMPT), second_dry, "greedy", breakers=breakers)
    assert np.array_equal(second, want) and touched_steps >= 1     # (80 steps, the loop starts near index 48 and the 3-gram ban ends it at once)
    assert _repeated(second.tolist(), 3) == 0
    t.set_dry_breakers([1024])                                   # the vocabulary is 1024
    t.reset(PROMPT)
    assert L.q4_run_transformer(1, C.byref(t.config), t.state, t.weights, 0, t.sampler) == ERR_ARG
    assert L.q4_run_transformer(0, C.byref(t.config), t.state, t.weights, 0, t.sampler) == 0      # a prompt step launches nothing
    t.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. log-probability records
@pytest.mark.parametrize("mode", ["greedy", "sampled"])
def test_records_describe_the_raw_logits(q4, paths, runs, mode):
    """with logprobs = 5 and DRY on, the records are those of a DRY-off model teacher-forced over the same ring: the top order of the raw logits, and
    the log-probability of the token the step chose under them (a greedy step's token is no longer entry 0 of the raw order)"""
    r = runs[mode]
    steps, k = 60, 5
    t = q4.Transformer(paths["small"], dry=DRY_FOR[mode], logprobs=k, **_sampler(mode))
    toks = t.generate_ids(PROMPT, steps)[0].copy()
    tlp, ids, top = t.logprobs(len(PROMPT) - 1, steps - len(PROMPT) + 1)
    t.close()
    assert np.array_equal(toks, r["tokens"][:steps + 1])
    t = q4.Transformer(paths["small"], logprobs=k)
    t.reset(toks)
    for pos in range(steps):
        t.run_transformer_at(pos, 0)
    wtlp, wids, wtop = t.logprobs(len(PROMPT) - 1, steps - len(PROMPT) + 1)
    t.close()
    assert np.array_equal(ids, wids)
    print("%s: largest difference top %g, token %g" % (mode, np.abs(top - wtop).max(), np.abs(tlp - wtlp).max()))
    assert np.array_equal(top, wtop)
    assert np.array_equal(tlp, wtlp)
    chosen_is_not_first = sum(int(toks[p + 1]) != int(wids[p - len(PROMPT) + 1][0]) for p in range(len(PROMPT) - 1, steps))
    assert chosen_is_not_first >= 1, "every step chose the raw logits' largest: the look-up behind the argmax was not exercised"


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. no state
@pytest.mark.parametrize("mode", ["greedy", "sampled"])
def test_a_resumed_generation_gives_the_full_runs_tokens(q4, paths, runs, mode):
    """generate_ids(prompt, steps, reuse=<Snapshot>) from position 119 of another model's rows: nothing of DRY has to be carried over"""
    r = runs[mode]
    t = q4.Transformer(paths["small"], dry=DRY_FOR[mode], **_sampler(mode))
    assert np.array_equal(t.generate_ids(PROMPT, 160)[0], r["tokens"][:161])
    snap = t.snapshot(119)
    t.close()
    t = q4.Transformer(paths["small"], dry=DRY_FOR[mode], **_sampler(mode))
    got = t.generate_ids(r["tokens"][:120], STEPS, reuse=snap)
    assert got[2] == STEPS - 1 - 119, "the prefix was not reused"
    assert np.array_equal(got[0], r["tokens"])
    t.close()
    snap.close()


def test_a_shifted_context_needs_no_bookkeeping(q4, paths):
    """two models teacher-forced identically, shifted by q4_shift_context(keep 4, discard 64) and stepped once, one with DRY off and one with DRY on:
    the second one's processed logits are the reference over the first one's logits and the SHIFTED ring"""
    ring = np.array(([1] + [5, 9, 17] * 70)[:201], dtype=np.int32)
    got = {}
    for how in ("off", "on"):
        t = q4.Transformer(paths["small"], dry=DRY if how == "on" else None)
        t.reset(ring)
        for pos in range(200):
            t.run_transformer_at(pos, 0)
        q4.synchronize()
        t.shift_context(4, 64)
        assert t.pos() == 136
        t.run_transformer(1)
        q4.synchronize()
        got[how] = (t.logits(), np.array([t.token(i) for i in range(137)], dtype=np.int32))
        t.close()
    assert np.array_equal(got["off"][1], got["on"][1]) and np.array_equal(got["on"][1], np.concatenate([ring[:4], ring[68:201]]))
    want, touched = _want(q4, got["off"][0], got["on"][1], 136, DRY)
    assert touched and got["on"][0].tobytes() == want.tobytes() != got["off"][0].tobytes()


# ---------------------------------------------------------------------------------------------------------------------------------
# the neighbours: the screen, the executable
def test_greedy_steps_are_not_screened_while_dry_is_on(q4, tmp_path):
    path = str(tmp_path / "cls.bin")
    synth.write_model(path, "cls4096_ragged", seed=31)
    t = q4.Transformer(path, dry=DRY)
    t.generate_ids([1, 20, 300], 24)
    assert t.screen_candidates()[3] == 0
    t.set_dry()
    t.generate_ids([1, 20, 300], 24)
    assert t.screen_candidates()[3] > 0, "the model does not screen at all: the check above shows nothing"
    t.close()


def test_cli_reads_the_environment_variables():
    """Q4_DRY and Q4_DRY_BREAKERS through the built executable on the committed micro model, greedy (its plain run repeats a 2-gram near the end)"""
    exe = os.path.join(ROOT, "llama_cu_awq_amd", "bin", "llama2_q4")
    args = [exe, os.path.join(GOLDEN, "micro_model.bin"), "-n", "32", "-i", "Hello", "-t", "0", "-s", "42", "-z", os.path.join(GOLDEN, "tokenizer.bin")]
    env = {k: v for k, v in os.environ.items() if k not in ("Q4_DRY", "Q4_DRY_BREAKERS")}
    strip = lambda s: re.sub(r"achieved tok/s.*", "", s)
    run = lambda e: subprocess.run(args, capture_output=True, text=True, timeout=300, errors="replace", env=e)
    plain = run(env)
    on = run(dict(env, Q4_DRY="ngram=2,last_n=64"))
    again = run(dict(env, Q4_DRY="ngram=2,last_n=64", Q4_DRY_BREAKERS="default"))
    assert plain.returncode == 0 and on.returncode == 0 and again.returncode == 0, (plain.stderr, on.stderr, again.stderr)
    assert strip(on.stdout) == strip(again.stdout)               # the ban ignores breakers
    assert strip(on.stdout) != strip(plain.stdout)
    assert strip(run(dict(env, Q4_DRY="")).stdout) == strip(plain.stdout)
    bad = run(dict(env, Q4_DRY="ngram=1"))
    assert bad.returncode != 0 and "Q4_DRY" in bad.stderr
    bad = run(dict(env, Q4_DRY="multiplier=0.8", Q4_DRY_BREAKERS="13,x"))
    assert bad.returncode != 0 and "Q4_DRY_BREAKERS" in bad.stderr
