"""typical-p, top-n-sigma and Mirostat v2 inside the decode step (csrc/q4_adaptive.hip, q4_sampler_set_adaptive, q4_adaptive_mask).
The threshold contract (tests/adaptive_ref.py): (1) the thresholds a launch RECORDS are held to the float64 restatement -- lse, lse_t, mu and T_m to
bounds derived from the arithmetic, T_s, H and d* to 4 x the worst deviation measured on the GPU over these very cases
(tools/measure_adaptive_parity.py -> profiles/adaptive_parity.json); (2) the mask is EXACTLY what those recorded thresholds say, recomputed in numpy
float32, no entry and no band left out; (3) typical-p's kept set is minimal in float64; (4) untouched entries keep their bits; (5) two launches give
the same bytes. Then the launch inside the step: every graph form against eager mode, values that change without a capture, the masks of four
launches nesting, context shift, resume, off after on, Mirostat at temperature 0."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import adaptive_ref as ref
from conftest import ROOT
from llama_cu_awq_amd import synth

pytestmark = pytest.mark.gpu

ERR_ARG = 5
F, D = np.float32, np.float64
with open(os.path.join(ROOT, "profiles", "adaptive_parity.json")) as _f:
    MEASURED = json.load(_f)["worst"]                            # {"T_s": ..., "H": ..., "d_star": ...}, |kernel - float64| / max(1, |float64|)
SLACK = 4.0                                                      # rounding-order slack on the measured deviations


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float16).view(np.uint16)


class Op:
    """device buffers for q4_adaptive_mask at vocabulary n and a ring of `positions`"""

    def __init__(self, q4, n, positions=8):
        self.q4, self.n = q4, n
        self.logits, self.rec = q4.DevBuf(nbytes=2 * n), q4.DevBuf(nbytes=4 * q4.ADAPTIVE_RECORD)
        self.mu, self.side = q4.DevBuf(nbytes=4 * positions), q4.DevBuf(nbytes=4 * (n + 2))
        self.tokens, self.pos = q4.DevBuf(nbytes=4 * positions), q4.DevBuf(nbytes=4)
        self.positions = positions
        self.clear()

    def clear(self):
        self.mu.put(np.full(self.positions, np.nan, dtype=F))
        side = np.full(self.n + 2, -np.inf, dtype=F)
        side[self.n:] = np.array([-1], dtype=np.int32).view(F)[0], np.nan
        self.side.put(side)

    def launch(self, x, c, temperature, pos=0, tok=0):
        q4 = self.q4
        self.logits.put(x)
        self.rec.put(np.full(q4.ADAPTIVE_RECORD, 7.0, dtype=F))
        self.pos.put(np.array([pos], dtype=np.int32))
        ring = np.zeros(self.positions, dtype=np.int32)
        ring[pos] = tok
        self.tokens.put(ring)
        q4.adaptive_mask(self.logits, self.n, temperature=temperature, mu_ring=self.mu, side=self.side, tokens=self.tokens, pos=self.pos,
                         record=self.rec, **c)
        q4.synchronize()
        return self.logits.get(np.float16, self.n), q4.adaptive_record(self.rec.get(F, q4.ADAPTIVE_RECORD))


def _check(what, x, got, rec, c, temperature, chain=None, pos=0, tok=None, mu_tol=0.0):
    """checks 1 - 4 of one launch"""
    want_out, dev, bounded, minimal = ref.staged(x, rec, c, temperature, chain if chain is not None else ref.Chain(), pos, tok, mu_tol)
    for name, g, w, tol in bounded:                              # 1. derived bounds
        print("%s: %s %.9g, float64 %.9g, |difference| %.3g, bound %.3g" % (what, name, g, w, abs(g - w), tol))
        assert abs(g - w) <= tol, "%s: %s %.9g against %.9g, bound %.3g" % (what, name, g, w, tol)
    for name, v in dev.items():                                  # 1. measured x 4
        print("%s: %s deviates %.3g (measured worst %.3g)" % (what, name, v, MEASURED[name]))
        assert v <= SLACK * MEASURED[name], "%s: %s deviates %.3g from float64, allowed %.3g" % (what, name, v, SLACK * MEASURED[name])
    bad = np.nonzero(_bits(got) != _bits(want_out))[0]           # 2. the mask exactly, and 4. the bits of what stayed
    assert bad.size == 0, "%s: %d entries differ from the recorded thresholds' mask, first %d: got %04x, expected %04x (input %04x)" % (
        what, bad.size, bad[0], _bits(got)[bad[0]], _bits(want_out)[bad[0]], _bits(x)[bad[0]])
    changed = _bits(got) != _bits(x)
    assert (_bits(got)[changed] == ref.NEG_INF_BITS).all() and np.isfinite(x.astype(F)[changed]).all(), what + ": something other than a mask was written"
    assert rec["kept"] == int(np.isfinite(got.astype(F)).sum()), what
    if minimal is not None:                                      # 3. minimality in float64
        tp = ref.controls(**c)["typical_p"]
        mass, inner, eps = minimal
        print("%s: kept mass %.9g, without the outermost tier %.9g, typical_p %.9g, eps %.3g" % (what, mass, inner, tp, eps))
        assert mass >= tp - eps, "%s: the kept mass %.9g is below typical_p %.9g" % (what, mass, tp)
        assert inner < tp + eps, "%s: the set without its outermost tier already holds %.9g >= typical_p %.9g" % (what, inner, tp)
    for k, on in (("T_s", c.get("top_n_sigma", 0) > 0), ("H", c.get("typical_p", 1) < 1), ("d_star", c.get("typical_p", 1) < 1)):
        if not on:
            assert np.isnan(rec[k]), "%s: %s recorded although its stage is off" % (what, k)
    return bounded


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. the op against the threshold contract
@pytest.mark.parametrize("n", ref.SIZES)
def test_op_holds_the_threshold_contract(q4, n):
    op = Op(q4, n)
    launches = highest = 0
    for name, x in ref.inputs(n):
        for cname, c, t in ref.CONFIGS:
            what = "n %d, %s, %s" % (n, name, cname)
            op.clear()
            got, rec = op.launch(x, c, t)
            mu, side = op.mu.get(F, op.positions), op.side.get(F, n + 2)
            _check(what, x, got, rec, c, t)
            if n > ref.HIGH:                                     # beyond 16 bits of id: on the mask the recorded thresholds give (the reference's answer)
                stays = np.flatnonzero(np.isfinite(ref.expect_from_record(x, rec, t)[0].astype(F)))
                v = x.astype(F)
                if stays.size < int(np.isfinite(v).sum()):       # (a Mirostat span's first position masks nothing: then only the maximum decides)
                    assert stays.size and stays.min() >= ref.HIGH, (what, stays[:4])
                    highest = max(highest, int(stays.max()))
                assert np.flatnonzero(v == np.nanmax(v)).min() >= ref.HIGH, what
            if c.get("mirostat_tau", 0) > 0:                     # a span starts: 2 * tau, written to the ring; the side buffer is w of what stayed
                assert rec["mu"] == F(2.0) * F(c["mirostat_tau"]) and mu[0] == rec["mu"] and np.isnan(mu[1:]).all(), what
                if np.isfinite(got.astype(F)).any():
                    w = got.astype(F) / F(t)
                    assert np.array_equal(side[:n], np.where(np.isfinite(w), w, F(-np.inf))), what + ": the side buffer"
                    assert side[n:n + 1].view(np.int32)[0] == 0 and abs(D(side[n + 1]) - ref.lse64(w[np.isfinite(w)])) <= ref.lse_bound(w), what
                else:
                    assert side[n:n + 1].view(np.int32)[0] == -1, what
            else:
                assert np.isnan(rec["mu"]) and np.isnan(rec["T_m"]) and np.isnan(mu).all(), what + ": Mirostat is off"
            op.clear()
            again, rec2 = op.launch(x, c, t)                     # 5. the same bytes
            assert again.tobytes() == got.tobytes() and all(np.array_equal(np.array(rec[k]), np.array(rec2[k]), equal_nan=True) for k in rec), what
            launches += 1
    assert launches == 30
    assert n <= ref.HIGH or highest > 98304, highest


def test_op_without_mirostat_needs_no_state(q4):
    n = 1000
    x = ref.inputs(n)[0][1]
    dl, dr = q4.DevBuf(x), q4.DevBuf(nbytes=4 * q4.ADAPTIVE_RECORD)
    q4.adaptive_mask(dl, n, typical_p=0.9, top_n_sigma=2.0, record=dr)
    q4.synchronize()
    got, rec = dl.get(np.float16, n), q4.adaptive_record(dr.get(F, q4.ADAPTIVE_RECORD))
    _check("no state", x, got, rec, dict(typical_p=0.9, top_n_sigma=2.0), 1.0)
    dl.put(x)
    q4.adaptive_mask(dl, n, typical_p=0.9, top_n_sigma=2.0)       # ... nor a record
    q4.synchronize()
    assert dl.get(np.float16, n).tobytes() == got.tobytes() != x.tobytes()
    dl.put(x)
    q4.adaptive_mask(dl, n)                                       # everything neutral: no launch
    q4.synchronize()
    assert dl.get(np.float16, n).tobytes() == x.tobytes()


@pytest.mark.parametrize("n", [1000, 32776])
def test_mirostat_chain_at_op_level(q4, n):
    """five consecutive positions, crafted logits, chosen tokens: mu against float64 within the propagated tolerance; the span start; a stale
    side_pos; the argmax entry under a mu below its own surprise"""
    rng = np.random.default_rng(77 + n)
    c, t = dict(mirostat_tau=3.0, mirostat_eta=0.4), 0.8
    op, chain = Op(q4, n), ref.Chain()
    mu_tol, mus = 0.0, []
    for pos in range(5):
        x = (rng.standard_normal(n) * 2.0).astype(np.float16)
        x[(7 * pos + 3) % n] = 9.0                               # one likely token and a long tail
        tok = None
        if pos > 0:                                              # the "sampler" takes: the likely token, an entry in the tail of what stayed, a masked one
            kept = np.nonzero(np.isfinite(chain.side))[0]
            tok = int(kept[np.argsort(chain.side[kept])[[-1, len(kept) // 2, 0, -1][pos - 1]]])
            if pos == 4:
                tok = int(np.nonzero(~np.isfinite(chain.side))[0][0])      # ... which has no surprise: mu stays
            if np.isfinite(chain.side[tok]):
                mu_tol = ref.mu_tolerance(mu_tol, c["mirostat_eta"], c["mirostat_tau"], chain.side_lse, chain.side[tok], chain.mu[pos - 1])
        got, rec = op.launch(x, c, t, pos, tok or 0)
        _check("n %d, position %d" % (n, pos), x, got, rec, c, t, chain, pos, tok, mu_tol)
        mus.append(rec["mu"])
    assert mus[0] == F(6.0) and mus[4] == mus[3] and len(set(mus[:4])) == 4, mus
    assert np.array_equal(op.mu.get(F, 5), np.array(mus, dtype=F))
    # a stale side buffer (a rewind: the launch at position 2 again, the side buffer describes position 4): mu[2] = mu[1]
    x = (rng.standard_normal(n) * 2.0).astype(np.float16)
    got, rec = op.launch(x, c, t, 2, 5)
    assert rec["mu"] == mus[1], (rec["mu"], mus)
    # mu below the argmax's own surprise: T_m lies above every entry and the largest w, lowest index, stays alone
    op.clear()
    flat = np.zeros(n, dtype=np.float16)
    flat[[n // 2, n - 1]] = 0.5
    got, rec = op.launch(flat, dict(mirostat_tau=0.25, mirostat_eta=0.4), t, 0, 0)
    assert np.nonzero(np.isfinite(got.astype(F)))[0].tolist() == [n // 2] and rec["kept"] == 1 and rec["T_m"] > F(0.5) / F(t)
    assert op.side.get(F, n + 2)[n // 2] == F(0.5) / F(t)


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. inside the step
PROMPT = [1, 5, 9]
STEPS = 40
SEED = 4242
ALL = dict(typical_p=0.95, top_n_sigma=3.0, mirostat_tau=4.0, mirostat_eta=0.2)


@pytest.fixture(scope="module")
def path(tmp_path_factory):
    p = str(tmp_path_factory.mktemp("adaptive") / "small.bin")
    synth.write_model(p, "small", seed=7)
    return p


def _run(q4, path, topp, adaptive, mode=1, steps=STEPS):
    L = q4.lib()
    L.q4_set_use_graphs(mode)
    try:
        t = q4.Transformer(path, temperature=0.8, topp=topp, seed=SEED, adaptive=adaptive)
        toks = t.generate_ids(PROMPT, steps)[0].copy()
        recs = t.adaptive_records(0, steps) if adaptive else None
        t.close()
    finally:
        L.q4_set_use_graphs(1)
    return toks, recs


@pytest.mark.parametrize("topp", [1.0, 0.9])
def test_graphs_equal_eager_bit_for_bit(q4, path, topp):
    """tokens and the record ring under the eight-steps-per-replay graphs against eager mode 2; the records are what the rule says they must be"""
    toks, recs = _run(q4, path, topp, ALL)
    etoks, erecs = _run(q4, path, topp, ALL, mode=2)
    assert len(toks) == STEPS + 1, "the run stopped at an EOS: pick another seed"
    assert np.array_equal(toks, etoks), "first difference at %d" % int(np.nonzero(toks != etoks)[0][0])
    assert recs.tobytes() == erecs.tobytes()
    plain = _run(q4, path, topp, None)[0]
    assert not np.array_equal(plain, toks), "the truncation changed nothing"
    gen = len(PROMPT) - 1                                        # the first generating position
    assert np.isnan(recs[:gen]).all() and not np.isnan(recs[gen:STEPS, :5]).any()
    mu = recs[:, 3]
    assert mu[gen] == F(2.0) * F(ALL["mirostat_tau"]) and len(set(mu[gen:STEPS].tolist())) > STEPS // 2, mu
    kept = recs[gen:STEPS, 5].copy().view(np.int32)
    assert (kept >= 1).all() and (kept < 1024).any()


def test_values_change_without_a_capture_and_on_off_captures_once(q4, path):
    L = q4.lib()
    t = q4.Transformer(path, temperature=0.8, topp=1.0, seed=SEED)
    c0 = L.q4_graph_captures()
    plain = t.generate_ids(PROMPT, STEPS)[0].copy()
    c_plain = L.q4_graph_captures() - c0
    t.set_adaptive(**ALL)
    on = t.generate_ids(PROMPT, STEPS)[0].copy()
    c_on = L.q4_graph_captures() - c0 - c_plain
    assert c_plain > 0 and c_on > 0                              # off -> on: the variants with the launch are captured
    t.set_adaptive(typical_p=0.5, mirostat_tau=2.0, mirostat_eta=0.5)      # other values, a stage less: the same graphs
    other = t.generate_ids(PROMPT, STEPS)[0].copy()
    recs = t.adaptive_records(0, STEPS)
    assert L.q4_graph_captures() - c0 == c_plain + c_on, "a change of values captured again"
    assert recs[len(PROMPT) - 1, 3] == F(4.0) and np.isnan(recs[len(PROMPT) - 1, 0]), "the new values did not reach the launch"
    assert len(plain) == len(on) == len(other) == STEPS + 1
    t.set_adaptive()                                             # on -> off: the plain graphs are still there
    t.generate_ids(PROMPT, STEPS)
    assert L.q4_graph_captures() - c0 == c_plain + c_on
    t.set_adaptive(**ALL)                                        # ... and so are the others
    t.generate_ids(PROMPT, STEPS)
    assert L.q4_graph_captures() - c0 == c_plain + c_on
    assert t.adaptive_records(len(PROMPT) - 1, 1)[0, 3] == F(8.0)
    t.close()


def test_off_after_on_equals_a_process_that_never_touched_it(q4, path):
    """the second of two runs of one Transformer (the sampler draws one coin per step, so both processes have drawn as many): here the first ran with
    the launch on, in the child process nothing ever called a setter"""
    t = q4.Transformer(path, temperature=0.8, topp=0.9, seed=SEED, adaptive=ALL)
    assert len(t.generate_ids(PROMPT, STEPS)[0]) == STEPS + 1
    t.set_adaptive()
    off = t.generate_ids(PROMPT, STEPS)[0].copy()
    t.close()
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from llama_cu_awq_amd import api\n"
            "import ctypes as C\n"
            "L = api.lib(); api.check(L.q4_set_device(0)); s = C.c_void_p(); api.check(L.q4_stream_create(C.byref(s))); L.q4_set_stream(s)\n"
            "t = api.Transformer(%r, temperature=0.8, topp=0.9, seed=%d)\n"
            "assert len(t.generate_ids(%r, %d)[0]) == %d\n"
            "print('TOKENS', ' '.join(str(int(v)) for v in t.generate_ids(%r, %d)[0]))\n"
            "t.close()\n" % (ROOT, path, SEED, PROMPT, STEPS, STEPS + 1, PROMPT, STEPS))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    line = [ln for ln in out.stdout.splitlines() if ln.startswith("TOKENS ")][0]
    assert off.tolist() == [int(v) for v in line.split()[1:]]


def test_masks_nest_behind_guide_dry_and_top_k(q4, path):
    """a guide, DRY, top-k 40 and this launch in one greedy step: what the launches in front masked stays -inf, what this launch leaves keeps the bits
    they left (after a greedy generating step RunState::logits holds the processed logits)"""
    V = 1024                                                     # synth model `small`
    table = np.zeros((1, V), dtype=np.uint16)
    table[0, 1::2] = q4.GUIDE_DEAD                               # one state: even tokens only
    g = q4.Guide(table)
    ring = [1, 6, 8, 6, 8, 6]
    kw = dict(guide=g, dry=dict(multiplier=0.8, base=1.75, allowed_length=1, last_n=64), sampling=dict(top_k=40))
    logits = {}
    for name, adaptive in (("front", None), ("all", dict(typical_p=0.6, top_n_sigma=1.0))):
        t = q4.Transformer(path, adaptive=adaptive, **kw)
        assert t.config.vocab_size == V
        t.reset(ring)
        for pos in range(len(ring)):
            t.run_transformer_at(pos, pos >= len(ring) - 1)
        q4.synchronize()
        logits[name] = t.logits()
        if adaptive:
            rec = q4.adaptive_record(t.adaptive_records(len(ring) - 1, 1)[0])
        t.close()
    g.close()
    front, both = logits["front"], logits["all"]
    dead = np.isneginf(front.astype(F))
    assert dead[1::2].all() and int((~dead).sum()) == 40
    assert np.isneginf(both.astype(F))[dead].all(), "an entry the launches in front masked came back"
    live = np.isfinite(both.astype(F))
    assert 1 <= live.sum() < 40 and _bits(both)[live].tobytes() == _bits(front)[live].tobytes()
    _check("behind guide, DRY and top-k", front, both, rec, dict(typical_p=0.6, top_n_sigma=1.0), 1.0)


def test_shift_moves_the_ring_entry_as_specified(q4, path):
    c = dict(mirostat_tau=4.0, mirostat_eta=0.2)
    t = q4.Transformer(path, temperature=0.8, topp=1.0, seed=SEED, adaptive=c)
    toks = t.generate_ids(PROMPT, STEPS)[0].copy()
    assert len(toks) == STEPS + 1
    n_pos = STEPS
    before = t.adaptive_records(0, n_pos)
    keep, discard = 4, 10
    t.shift_context(keep, discard, n_pos=n_pos)
    after = t.adaptive_records(0, n_pos)
    assert after[:keep].tobytes() == before[:keep].tobytes()
    assert after[keep:n_pos - discard].tobytes() == before[keep + discard:n_pos].tobytes()      # the rows moved with their positions
    assert after[n_pos - discard - 1, 3] == before[n_pos - 1, 3] and not np.isnan(before[n_pos - 1, 3])
    # the next generating step continues the chain from the moved entry: the side buffer's position was rebased with it
    t.run_transformer_at(n_pos - discard, 1)
    nxt = q4.adaptive_record(t.adaptive_records(n_pos - discard, 1)[0])
    assert not np.isnan(nxt["mu"]) and nxt["mu"] != F(8.0) and nxt["mu"] != before[n_pos - 1, 3]
    t.close()


def test_shift_of_a_long_ring_moves_every_row(q4, path):
    """300 positions, keep 4, discard 1: 295 rows (9.4 KB of records) move down by ONE row -- source and destination overlap almost entirely -- and
    every moved row is checked, as is every row that stays"""
    steps = 300
    t = q4.Transformer(path, temperature=0.8, topp=1.0, seed=SEED, adaptive=dict(mirostat_tau=4.0, mirostat_eta=0.2))
    toks = t.generate_ids(PROMPT, steps)[0].copy()
    assert len(toks) == steps + 1, "the run stopped at an EOS: pick another seed"
    before = t.adaptive_records(0, steps)
    gen = len(PROMPT) - 1
    assert not np.isnan(before[gen:, 3]).any() and len(set(before[gen:, 3].tolist())) > steps // 2      # (rows that differ: a misplaced one shows)
    keep, discard = 4, 1
    t.shift_context(keep, discard, n_pos=steps)
    after = t.adaptive_records(0, steps)
    assert after[:keep].tobytes() == before[:keep].tobytes()
    moved, want = after[keep:steps - discard], before[keep + discard:steps]
    bad = np.nonzero((moved.view(np.uint32) != want.view(np.uint32)).any(axis=1))[0]
    assert bad.size == 0, "%d of %d moved rows differ, first at position %d" % (bad.size, moved.shape[0], keep + bad[0])
    assert after[steps - discard:].tobytes() == before[steps - discard:].tobytes()      # behind the new position nothing was written
    t.run_transformer_at(steps - discard, 1)                     # the chain continues from the moved entry
    nxt = q4.adaptive_record(t.adaptive_records(steps - discard, 1)[0])
    assert not np.isnan(nxt["mu"]) and nxt["mu"] != F(8.0)
    t.close()


def test_a_resume_restarts_the_span(q4, path):
    c = dict(mirostat_tau=4.0, mirostat_eta=0.2)
    t = q4.Transformer(path, temperature=0.8, topp=1.0, seed=SEED, adaptive=c)
    toks = t.generate_ids(PROMPT, STEPS)[0].copy()
    full = t.adaptive_records(0, STEPS)
    start = 12
    assert full[start, 3] != F(8.0)                              # (in the full run the chain had moved on by then)
    t.generate_ids_from(toks[:start + 1], start + 8, start)      # the rows of [0, start) are in place; steps counts positions
    recs = t.adaptive_records(0, start + 4)
    assert np.isnan(recs[:start, 3]).all() and recs[start, 3] == F(8.0) and not np.isnan(recs[start + 1:start + 4, 3]).any()
    t.close()


def test_mirostat_at_temperature_0_is_an_argument_error(q4, path):
    t = q4.Transformer(path, temperature=0.0, adaptive=dict(mirostat_tau=5.0))
    t.reset(PROMPT)
    L = q4.lib()
    for pos in range(len(PROMPT) - 1):
        t.run_transformer_at(pos, 0)                             # prompt steps launch nothing: no error yet
    rc = L.q4_run_transformer_at(len(PROMPT) - 1, 1, C.byref(t.config), t.state, t.weights, 0, t.sampler)
    assert rc == ERR_ARG
    t.set_adaptive(typical_p=0.9)                                # greedy with the other stages runs
    t.run_transformer_at(len(PROMPT) - 1, 1)
    q4.synchronize()
    assert q4.adaptive_record(t.adaptive_records(len(PROMPT) - 1, 1)[0])["kept"] >= 1
    t.close()
