"""A generating step with the guide, DRY, the sampling controls and the adaptive truncation all on, against ONE composed reference
(tests/logit_chain_ref.py: the four references in the order of csrc/q4_step.hip's STAGES table) over the raw logits of a plain model teacher-forced
along the run's own ring: every sampled token is the restated sampler's over the composed logits with that position's coin, every greedy token the
lowest-index argmax, and the processed logits the last greedy step leaves are the composed ones bit for bit. The adaptive stage is held the way
tests/test_adaptive_gpu.py holds it (recorded thresholds against float64 within the committed bounds, the mask exact from the recorded thresholds); no
tolerance is new here. The same test shows ON THE CPU that it can tell the order: the first three stages recomputed in two other orders differ from
the right one in some generating step of every run. Then the check across a resume and across q4_shift_context."""
import ctypes as C

import numpy as np
import pytest

import adaptive_ref
import guide_ref
import logit_chain_ref as ref
import sampling_controls_ref
import teacher_forced
from llama_cu_awq_amd import synth
from test_adaptive_gpu import MEASURED, SLACK
from test_logit_stages_gpu import ROUNDS as STAGE_ROUNDS, SamplerStruct, V, _guide

pytestmark = pytest.mark.gpu

PROMPT = [1, 5, 9]
STEPS = 40                       # positions 0, 1 feed the prompt; 2 .. 33 go out as four eight-step replays, 34 .. 39 one by one
SEED = 4242
SAMPLED = (0.5, 0.9)
F, D = np.float32, np.float64
# The stage test's two rounds and one with Mirostat off. A run tells "DRY, then the controls" from "the controls, then DRY" only where DRY touches an entry
# that the controls treat too, so the second and third rounds are strengthened for that: a prompt that repeats itself inside the DRY window (at the
# first generating step the token 8 follows an earlier occurrence of the ring's last token) and a bias that keeps 8 among the top-k entries.
ROUNDS = [
    dict(STAGE_ROUNDS[0], prompt=PROMPT),
    dict(STAGE_ROUNDS[1], prompt=[1, 6, 8, 6, 8, 6], bias={**STAGE_ROUNDS[1]["bias"], 8: 3.0}),
    dict(dead_step=4, dry=dict(multiplier=1.0, base=1.5, allowed_length=1, last_n=32), sampling=dict(top_k=8, repeat_penalty=1.2, penalty_last_n=16),
         bias={8: 3.0, 12: -1.0}, adaptive=dict(typical_p=0.9, top_n_sigma=2.5), prompt=[1, 6, 8, 6]),
]
OTHER_ORDERS = (("guide", "controls", "dry"), ("dry", "controls", "guide"))


@pytest.fixture(scope="module")
def path(tmp_path_factory):
    p = str(tmp_path_factory.mktemp("chain") / "small.bin")
    synth.write_model(p, "small", seed=7)
    return p


def _adaptive(r, mode):
    a = dict(r["adaptive"])
    if mode == "greedy":                                         # (Mirostat at temperature 0 is an argument error)
        a.pop("mirostat_tau", None)
        a.pop("mirostat_eta", None)
    return a


def _model(q4, path, r, mode):
    t = q4.Transformer(path, **(dict(temperature=SAMPLED[0], topp=SAMPLED[1], seed=SEED) if mode == "sampled" else dict(temperature=0.0)))
    assert t.config.vocab_size == V
    g = _guide(q4, r["dead_step"])
    t.set_guide(g)
    t.set_dry(**r["dry"])
    t.set_sampling(**r["sampling"])
    t.set_logit_bias(r["bias"])
    t.set_adaptive(**_adaptive(r, mode))
    return t, g


def _table(r):
    table = np.zeros((1, V), dtype=np.uint16)
    table[0, 1::r["dead_step"]] = guide_ref.DEAD
    table[0, 2] = guide_ref.DEAD
    return table


def _coins(q4, n):
    state = C.c_ulonglong(SEED)
    return [q4.lib().random_f32(C.byref(state)) for _ in range(n)]


class Run:
    """the reference's state along one run: the guide's state ring, Mirostat's chain and the tolerance its mu has accumulated"""

    def __init__(self, q4, r, mode, n_positions):
        self.r, self.mode = r, mode
        self.adaptive = _adaptive(r, mode)
        self.table = _table(r)
        self.states = np.full(n_positions, guide_ref.NONE, dtype=np.int32)
        self.mirostat = adaptive_ref.Chain() if self.adaptive.get("mirostat_tau", 0) > 0 else None
        self.mu_tol = 0.0
        self.pen = q4.dry_penalty_table(multiplier=r["dry"]["multiplier"], base=r["dry"]["base"], allowed_length=r["dry"]["allowed_length"])
        self.told_apart = [0] * len(OTHER_ORDERS)

    def step(self, orc, what, raw16, ring, p, rec, coin):
        """composes position p and returns (the token the step must have chosen, the composed logits)"""
        r = self.r
        for k, order in enumerate(OTHER_ORDERS):                 # (before the right order: it writes the state ring)
            other = ref.front(raw16, ring, p, self.table, self.states.copy(), r["dry"], self.pen, r["sampling"], r["bias"], order)
            right = ref.front(raw16, ring, p, self.table, self.states.copy(), r["dry"], self.pen, r["sampling"], r["bias"])
            self.told_apart[k] += int(other.tobytes() != right.tobytes())
        if r["sampling"].get("min_p", 0) > 0:                    # (test_min_p_keeps_the_reference_set's condition on the inputs: two logf may differ in the last bit)
            x2 = ref.front(raw16, ring, p, self.table, self.states.copy(), r["dry"], self.pen, None, None)
            margin = sampling_controls_ref.min_p_margin(x2, tokens=ring, pos=p, logit_bias=r["bias"], **r["sampling"])
            assert margin > 2.0 ** -20, "%s: an entry within 2^-20 of the min-p threshold: pick another seed" % what
        temperature = SAMPLED[0] if self.mode == "sampled" else 1.0
        out, x3, dev, bounded, minimal, self.mu_tol = ref.chain(raw16, ring, p, self.table, self.states, r["dry"], self.pen, r["sampling"], r["bias"],
                                                                self.adaptive, rec, temperature, self.mirostat, self.mu_tol)
        for name, g, w, tol in bounded:                          # the adaptive stage's recorded thresholds: test_adaptive_gpu._check's bounds
            print("%s: %s %.9g, float64 %.9g, |difference| %.3g, bound %.3g" % (what, name, g, w, abs(g - w), tol))
            assert abs(g - w) <= tol, "%s: %s %.9g against %.9g, bound %.3g" % (what, name, g, w, tol)
        for name, v in dev.items():
            print("%s: %s deviates %.3g (measured worst %.3g)" % (what, name, v, MEASURED[name]))
            assert v <= SLACK * MEASURED[name], "%s: %s deviates %.3g from float64, allowed %.3g" % (what, name, v, SLACK * MEASURED[name])
        if minimal is not None:
            tp = adaptive_ref.controls(**self.adaptive)["typical_p"]
            mass, inner, eps = minimal
            assert mass >= tp - eps and inner < tp + eps, "%s: typical-p kept %.9g, %.9g without its outermost tier, typical_p %.9g" % (what, mass, inner, tp)
        kept = int(np.isfinite(out.astype(F)).sum())
        assert rec["kept"] == kept >= 1, "%s: the launch recorded %d kept entries, the composed reference leaves %d" % (what, rec["kept"], kept)
        assert np.isneginf(out.astype(F))[np.isneginf(x3.astype(F))].all()
        if self.mode == "greedy":
            return int(np.argmax(out.astype(F))), out
        return orc.lib().orc_sample_topp(orc.f16_bits(out.copy()), V, SAMPLED[0], SAMPLED[1], coin), out


def _check_positions(q4, orc, run, what, raw, ring, positions, recs, coins):
    bad, out = [], None
    for p in positions:
        rec = q4.adaptive_record(recs[p])
        tok, out = run.step(orc, "%s, position %d" % (what, p), raw[p], ring, p, rec, coins[p] if coins is not None else None)
        if tok != int(ring[p + 1]):
            bad.append("position %d: token %d, composed reference %d" % (p, int(ring[p + 1]), tok))
    assert not bad, "%s: %d of %d steps differ: %s" % (what, len(bad), len(positions), "; ".join(bad[:6]))
    return out


@pytest.mark.parametrize("mode", ["sampled", "greedy"])
@pytest.mark.parametrize("round_", range(len(ROUNDS)))
def test_every_step_is_the_composed_reference(q4, orc, path, round_, mode):
    r = ROUNDS[round_]
    what = "round %d %s" % (round_, mode)
    t, g = _model(q4, path, r, mode)
    try:
        ring = t.generate_ids(r["prompt"], STEPS)[0].copy()
        assert len(ring) == STEPS + 1, what + ": the run stopped at an EOS: pick another seed"
        recs, states, last = t.adaptive_records(0, STEPS), t.guide_states(0, STEPS), t.logits()
    finally:
        t.close()
        g.close()
    raw = teacher_forced.raw_logits(q4, path, ring)
    run = Run(q4, r, mode, STEPS)
    n_prompt = len(r["prompt"])
    gen = n_prompt - 1
    out = _check_positions(q4, orc, run, what, raw, ring, range(gen, STEPS), recs, _coins(q4, STEPS) if mode == "sampled" else None)
    assert np.array_equal(states, run.states), what + ": the guide's state ring"
    assert (ring[n_prompt:] % r["dead_step"] != 1).all() and (ring[n_prompt:] != 2).all(), what + ": a token the guide forbids"
    if mode == "greedy":         # after a greedy generating step RunState::logits holds the PROCESSED logits
        diff = np.nonzero(last.view(np.uint16) != out.view(np.uint16))[0]
        assert diff.size == 0, "%s: %d entries of the last step's logits differ from the composed reference, first %d: %04x, reference %04x" % (
            what, diff.size, diff[0], last.view(np.uint16)[diff[0]], out.view(np.uint16)[diff[0]])
    elif run.mirostat is not None:
        assert recs[gen, 3] == F(2.0) * F(r["adaptive"]["mirostat_tau"]) and len(set(recs[gen:, 3].tolist())) > STEPS // 2, what + ": mu does not move"
    assert len(set(ring[n_prompt:].tolist())) > 4, what + ": a constant ring shows nothing"
    for order, steps in zip(OTHER_ORDERS, run.told_apart):
        print("%s: the order %s differs from the step's in %d of %d generating steps" % (what, order, steps, STEPS - gen))
        assert steps >= 1, "%s: the order %s leaves the same logits in every step: the run cannot tell the orders apart (strengthen the round)" % (what, order)


def test_the_chain_across_a_resume(q4, orc, path):
    """generate_ids_from at position 12 of a finished run, Mirostat on: the guide starts at state 0 and Mirostat's span at 2 tau THERE, the coins are
    the full run's by position, and every step from 12 on is the composed reference over the new ring"""
    r, start, steps = ROUNDS[0], 12, 30
    t, g = _model(q4, path, r, "sampled")
    try:
        full = t.generate_ids(PROMPT, STEPS)[0].copy()
        assert len(full) == STEPS + 1
        C.cast(t.sampler, C.POINTER(SamplerStruct)).contents.rng_state = SEED
        ring = t.generate_ids_from(full[:start + 1], steps, start)[0].copy()
        assert len(ring) == steps + 1 and np.array_equal(ring[:start + 1], full[:start + 1])
        recs, states = t.adaptive_records(0, steps), t.guide_states(0, steps)
    finally:
        t.close()
        g.close()
    raw = teacher_forced.raw_logits(q4, path, ring)
    run = Run(q4, r, "sampled", steps)
    _check_positions(q4, orc, run, "resumed at %d" % start, raw, ring, range(start, steps), recs, _coins(q4, steps))
    assert np.array_equal(states, run.states) and (states[:start] == guide_ref.NONE).all()
    assert np.isnan(recs[:start, 3]).all() and recs[start, 3] == F(2.0) * F(r["adaptive"]["mirostat_tau"])


def test_the_chain_across_a_context_shift(q4, orc, path):
    """q4_shift_context(keep 4, discard 10) behind 40 positions, then six generating steps one by one: the stages read the ring by position -- the
    reference reads the SHIFTED ring, its guide states and Mirostat chain moved down with the rows -- and the raw logits come from a plain model
    teacher-forced and shifted the same way"""
    r, keep, discard, more = ROUNDS[0], 4, 10, 6
    t, g = _model(q4, path, r, "sampled")
    try:
        full = t.generate_ids(PROMPT, STEPS)[0].copy()
        assert len(full) == STEPS + 1
        recs = t.adaptive_records(0, STEPS)
        t.shift_context(keep, discard, n_pos=STEPS)
        base = STEPS - discard
        assert t.pos() == base
        for _ in range(more):
            t.run_transformer(1)
            q4.synchronize()
        ring = np.array([t.token(i) for i in range(base + more + 1)], dtype=np.int32)
        recs2, states2 = t.adaptive_records(0, base + more), t.guide_states(0, base + more)
    finally:
        t.close()
        g.close()
    assert np.array_equal(ring[:base + 1], np.concatenate([full[:keep], full[keep + discard:]]))
    coins = _coins(q4, STEPS + more)
    run = Run(q4, r, "sampled", STEPS)
    gen = len(PROMPT) - 1
    _check_positions(q4, orc, run, "before the shift", teacher_forced.raw_logits(q4, path, full), full, range(gen, STEPS), recs, coins)
    # the reference's state moves down with the rows
    run.states = np.concatenate([run.states[:keep], run.states[keep + discard:], np.full(more, guide_ref.NONE, dtype=np.int32)])
    ref.rebase(run.mirostat, discard)
    assert np.array_equal(states2[:base], run.states[:base])
    assert recs2[keep:base].tobytes() == recs[keep + discard:STEPS].tobytes()
    plain = q4.Transformer(path)
    try:
        plain.reset(full)
        for pos in range(STEPS):
            plain.run_transformer_at(pos, 0)
        q4.synchronize()
        plain.shift_context(keep, discard, n_pos=STEPS)
        raw = {}
        for p in range(base, base + more):
            plain.resume(ring[:p + 1], p)
            plain.run_transformer_at(p, 0)
            raw[p] = plain.logits()
    finally:
        plain.close()
    shifted_coins = {p: coins[p + discard] for p in range(base, base + more)}      # one coin per step the sampler ran, whatever the position
    _check_positions(q4, orc, run, "behind the shift", raw, ring, range(base, base + more), recs2, shifted_coins)
    assert np.array_equal(states2, run.states)
