"""Prompt and verify passes for Llama-2-13B's shape (q4_set_pass_13b; csrc/prompt_pass.hip, csrc/spec_verify.hip, DESIGN.md 3.7 "13B"): dim 5120 as
forty 128-wide heads, hidden 13824 -- the layer twice with a context of 2304 (`k5120_pair`), and once with Llama-2's vocabulary (`k5120_cls`). A pass
restates the step's arithmetic, so "equal" always means BYTE-equal against the same library running per-token steps with the switch off on a fresh
Transformer: the token ring, every K / V row of every layer below the final position, the final logits, the position, the sampler's rng_state where
there is one. No tolerance anywhere; the one place with bounds holds the same bytes to the CPU restatement and the unrounded double forward under the
brackets of tests/test_pass_hostile_gpu.py, so byte equality is not the only evidence.

What a pass of this shape adds to Llama-2-7B's: K = 5120 is two whole k-slots and the shared half slot (units 128 .. 159 on lanes 0 - 31 for the even
column of a pair and on lanes 32 - 63 for the odd one, the term a product and a sum, the other half adding 0.f) in the q/k/v, o-proj and gate/up
launches; the norm over 640 chunk partials; the down projection as two k-parts of 216 = 3 x 64 + 24 units; attention over forty heads; the verify
classifier over ten pieces per row."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import cache_poison as cp
import hostile_models as hm
import hostile_ref
import pass_context_ref as ref
import spec_ref
import test_speculative_gpu as tsg
from conftest import ROOT
from llama_cu_awq_amd import synth
from test_hostile_network_gpu import DEFAULT_BOUND, DEFAULT_KV_BOUND, SEQ, _rel, _rms
from test_pass_logprobs_gpu import _records, _score
from test_prompt_ingest_gpu import _expected_passes

pytestmark = pytest.mark.gpu

NAME = "k5120_pair"
CLS = "k5120_cls"
WIDE7B = "pass_long"
SEED = 11
T = 8
GEN = 6
S = 2304                  # k5120_pair's context, and the bound the long tests raise the setting to
AHEAD = 8                 # PROMPT_PASS_MAX: how far above the final position a pass may have written
N_LONG = 2200
N_SPEC = 17
MIN = 4                   # the fewest positions a pass of this shape takes (csrc/prompt_pass.h, prompt_pass_min): a pass of 2 or 3 measured slower than the steps


@pytest.fixture(scope="module")
def models(tmp_path_factory):
    d = tmp_path_factory.mktemp("pass_13b")
    made = {}

    def get(name, trait=None):
        if (name, trait) not in made:
            made[name, trait] = str(d / ("%s_%s.bin" % (name, trait)))
            if trait is None:
                synth.write_model(made[name, trait], name, seed=SEED)
            elif trait == "gqa":       # the 13B layer with eight K / V heads: no checkpoint family has it, the admission must refuse it
                dim, hidden, layers, heads, _, vocab, seq, theta = synth.GEOMETRIES[NAME]
                synth.write_model(made[name, trait], (dim, hidden, 1, heads, 8, vocab, 300, theta), seed=SEED)
            else:
                hm.write_hostile_model(made[name, trait], name, trait, seed=SEED)
        return made[name, trait]
    return get


def _prompt(n, seed=5):
    r = np.random.default_rng(seed)
    return [1] + [int(x) for x in r.integers(3, 512, size=n - 1)]       # no EOS (2) inside


_LONG = _prompt(N_LONG)


def _passes(n_prompt, steps, bound, model_seq_len, start=0, mode=1, ingest=T):
    """tests/pass_context_ref.py's prompt_passes with this shape's minimum: [(pos, n)] of the prompt passes of a generation"""
    out = []
    pos = start
    last = min(n_prompt - 1, steps)
    while pos < last:
        n = min(last - pos, ingest, ref.bin_end(pos) - pos, min(max(bound, 256), model_seq_len) - pos)
        if n >= MIN and ref.covers(pos, n, bound, model_seq_len, mode):
            out.append((pos, n))
            pos += n
        else:
            pos += 1
    return out


def _at_least(drafter, n=MIN - 1):
    """the drafter as the token loop of this shape uses it: not asked for fewer than n drafts, a shorter answer dropped"""
    def fn(ring, room):
        d = list(drafter(ring, room)) if room >= n else []
        return d if len(d) >= n else []
    return fn


def _wrong(tok):
    w = (int(tok) + 1) % 512
    return w + 1 if w == 2 else w


def _run(q4, path, prompt, steps=None, on=True, ingest=T, graphs=1, bound=256, start=0, warm=None, poison=None, spec=None, drafter=None, rows=True, **kw):
    """One generation on a fresh Transformer: dict(tokens, k, v (the rows below the final position), logits, pos, passes, stats, rng, covers).
    warm: a prompt generated first (start > 0 reuses its prefix). poison: (pattern, first row) written behind the warm run; the rows from AHEAD above
    the final position must still hold it."""
    L = q4.lib()
    default = L.q4_get_prompt_ingest()
    timeouts = L.q4_handoff_timeouts()
    try:
        L.q4_set_use_graphs(graphs)
        L.q4_set_prompt_ingest(ingest)
        q4.set_pass_context(bound)
        t = q4.Transformer(path, pass_13b=on, **kw)
        try:
            assert t.pass_13b() == bool(on)
            if warm is not None:
                t.generate_ids(warm, len(warm) + GEN)
            if poison is not None:
                cp.poison(q4, t, poison[1], poison[0])
            if spec is not None:
                t.set_speculative(**spec)
            if drafter is not None:
                t.set_drafter(drafter)
            steps = len(prompt) + GEN if steps is None else steps
            before = L.q4_prompt_passes()
            toks = t.generate_ids_from(prompt, steps, start)[0].copy()
            out = {"passes": L.q4_prompt_passes() - before,
                   "covers": [int(L.q4_verify_covers(t.h, p, 4)) for p in (0, 40, 300, 600, 1100, 2100) if p + 4 < t.config.seq_len]}
            q4.check(L.q4_handoff_status(t.state))
            assert L.q4_handoff_timeouts() == timeouts
            pos = t.pos()
            out.update(tokens=toks, pos=pos, logits=t.logits().view(np.uint16).copy(), stats=t.spec_stats(), rng=tsg._rng_state(t))
            if rows and kw.get("kv", "fp16") == "fp16":
                out["k"], out["v"] = cp.read_rows(q4, t, 0, pos)
            if poison is not None and pos + AHEAD < t.config.seq_len:
                cp.assert_untouched(q4, t, pos + AHEAD, poison[0], "final position %d" % pos)
        finally:
            t.close()
    finally:
        L.q4_set_prompt_ingest(default)
        L.q4_set_use_graphs(1)
        q4.set_pass_context(256)
    return out


def _assert_same(a, b, what, rng=True):
    assert np.array_equal(a["tokens"], b["tokens"]), "%s: token rings differ: %s vs %s" % (what, a["tokens"][-12:], b["tokens"][-12:])
    assert a["pos"] == b["pos"], "%s: positions %d vs %d" % (what, a["pos"], b["pos"])
    for name in ("k", "v"):
        if name in a or name in b:
            assert a[name].shape == b[name].shape
            bad = np.argwhere((a[name] != b[name]).any(axis=2))
            assert bad.size == 0, "%s: %s rows differ, first (layer, position) %s" % (what, name.upper(), [tuple(int(i) for i in x) for x in bad[:8]])
    assert np.array_equal(a["logits"], b["logits"]), "%s: final logits differ in %d entries" % (what, int((a["logits"] != b["logits"]).sum()))
    assert not rng or a["rng"] == b["rng"], "%s: the Sampler's random state differs" % what


_OFF = {}


def _off(q4, models, n_prompt, graphs=1, name=NAME, trait=None):
    """the per-token run (prompt ingest off, the switch off), computed once per case and shared"""
    key = (name, trait, n_prompt, graphs)
    if key not in _OFF:
        _OFF[key] = _run(q4, models(name, trait), _LONG[:n_prompt], on=False, ingest=0, graphs=graphs)
        assert _OFF[key]["passes"] == 0
    return _OFF[key]


# ---- 1. off is today ----------------------------------------------------------------------------------------------------------------------------------------
def test_off_is_today(q4, models):
    """The switch off: no pass over a 64-token prompt, q4_verify_covers 0 everywhere, q4_verify_tokens refuses, the bytes of ingest off. On: the counter
    advances (without the feature it cannot), the probe reports the admission, and the bytes stay."""
    off = _off(q4, models, 64)
    plain = _run(q4, models(NAME), _LONG[:64], on=False, bound=S)
    assert plain["passes"] == 0 and plain["covers"] == [0] * 6
    _assert_same(off, plain, "switch off")
    on = _run(q4, models(NAME), _LONG[:64], bound=S)
    assert on["passes"] == len(_passes(64, 64 + GEN, S, S)) == 8
    assert on["covers"] == [1] * 6
    _assert_same(off, on, "switch on")
    t = q4.Transformer(models(NAME))
    try:
        assert not t.pass_13b() and not t.verify_covers(30, 4)
        t.generate_ids(_LONG[:31], 30)
        assert t.verify([5, 6, 7]) is None and t.pos() == 30          # Q4_NOT_ADMITTED: nothing ran
        t.set_pass_13b(True)
        assert t.pass_13b() and t.verify_covers(30, 4) and t.verify_covers(248, 7) and not t.verify_covers(249, 7) and not t.verify_covers(300, 3)
        assert t.verify_covers(30, MIN - 1) and not t.verify_covers(30, MIN - 2) and not t.verify_covers(30, 1)        # the minimum: four rows
        t.set_pass_13b(False)
        assert not t.pass_13b() and not t.verify_covers(30, 4)
    finally:
        t.close()


# ---- 2. prompt passes below 256 -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graphs", [1, 2, 0])
@pytest.mark.parametrize("n_prompt", [3, 9, 10, 17, 64, 250])
def test_prompt_passes_below_256(q4, models, n_prompt, graphs):
    """with graphs, with eager bins, without graphs. Three prompt tokens are two prompt-only positions, below this shape's minimum: steps; ten are a
    pass of eight and a step; 250 are 31 passes of eight and one step; the others end on a pass of 7 or 8"""
    off = _off(q4, models, n_prompt, graphs)
    on = _run(q4, models(NAME), _LONG[:n_prompt], graphs=graphs)
    want = {3: 0, 9: 1, 10: 1, 17: 2, 64: 8, 250: 31}[n_prompt]
    assert on["passes"] == len(_passes(n_prompt, n_prompt + GEN, 256, S, mode=graphs)) == want
    _assert_same(off, on, "%d prompt tokens, graphs %d" % (n_prompt, graphs))


@pytest.mark.parametrize("ingest", [2, 3, 4, 5, 6, 7])
def test_smaller_passes(q4, models, ingest):
    """every pass size: the token groups of the launches (three and two per group) are cut at every place; below the minimum of four no pass runs"""
    off = _off(q4, models, 64)
    on = _run(q4, models(NAME), _LONG[:64], ingest=ingest)
    assert on["passes"] == len(_passes(64, 64 + GEN, 256, S, ingest=ingest)) and (on["passes"] > 0) == (ingest >= MIN)
    _assert_same(off, on, "passes of %d" % ingest)


# ---- 3. beyond 256 ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_prompt", [257, 300, 520, 1030, N_LONG])
def test_long_prompt(q4, models, n_prompt):
    """the bound at the context: chunks of 64 / 128 / 256, every bin end (256, 512, 1024, 2048) crossed by the pass sequence"""
    off = _off(q4, models, n_prompt)
    on = _run(q4, models(NAME), _LONG[:n_prompt], bound=S)
    assert on["passes"] == len(_passes(n_prompt, n_prompt + GEN, S, S)) > 0
    _assert_same(off, on, "%d prompt tokens" % n_prompt)


@pytest.mark.parametrize("graphs", [2, 0])
def test_long_prompt_eager(q4, models, graphs):
    off = _off(q4, models, 1030, graphs)
    on = _run(q4, models(NAME), _LONG[:1030], graphs=graphs, bound=S)
    assert on["passes"] == len(_passes(1030, 1030 + GEN, S, S, mode=graphs)) > 0
    _assert_same(off, on, "1030 prompt tokens, graphs %d" % graphs)


# ---- 4. verify passes ---------------------------------------------------------------------------------------------------------------------------------------
def _stepwise(q4, path, p, D=7, prompt=None, **kw):
    """prompt[:p + 1] stepped to position p, then D + 1 generating steps one by one: the true continuation R[p + 1 .. p + D + 1], and behind step i the
    logits, the position and rng_state; the rows [0, p + D + 1) at the end"""
    L = q4.lib()
    L.q4_set_prompt_ingest(0)
    t = q4.Transformer(path, **kw)
    try:
        t.generate_ids((prompt or _LONG)[:p + 1], p)
        assert t.pos() == p
        logits, rng = [], []
        for i in range(D + 1):
            t.run_transformer(True)
            q4.synchronize()
            assert t.pos() == p + i + 1
            logits.append(t.logits().view(np.uint16).copy())
            rng.append(tsg._rng_state(t))
        q4.check(L.q4_handoff_status(t.state))
        k, v = cp.read_rows(q4, t, 0, p + D + 1)
        return {"R": [t.token(i) for i in range(p + D + 2)], "logits": logits, "k": k, "v": v, "rng": rng}
    finally:
        t.close()
        L.q4_set_prompt_ingest(T)


def _set_rng(t, state):
    C.cast(t.sampler, C.POINTER(tsg.SamplerStruct)).contents.rng_state = state


def _stepwise_sampled(q4, path, p, D, seed, **kw):
    """_stepwise under the sampler: for k = 0 .. D one per-token generation of p + k + 1 steps from the seed's stream (a position's coin depends on the
    position alone, so the shorter runs are prefixes of the longest): behind each the probabilities a sampled step leaves and rng_state"""
    L = q4.lib()
    L.q4_set_prompt_ingest(0)
    t = q4.Transformer(path, seed=seed, **kw)
    try:
        logits, rng, rings = [], [], []
        for k in range(D + 1):
            _set_rng(t, seed)
            rings.append([int(x) for x in t.generate_ids(_LONG[:p + 1], p + k + 1)[0]])
            assert t.pos() == p + k + 1 and rings[-1][:len(rings[0])] == rings[0]
            logits.append(t.logits().view(np.uint16).copy())
            rng.append(tsg._rng_state(t))
        q4.check(L.q4_handoff_status(t.state))
        k, v = cp.read_rows(q4, t, 0, p + D + 1)
        return {"R": rings[-1], "logits": logits, "k": k, "v": v, "rng": rng}
    finally:
        t.close()
        L.q4_set_prompt_ingest(T)


def _verify_all_indices(q4, path, p, want, D=7, poison=None, sampled=False, vocab=512, **kw):
    """q4_verify_tokens (sampled: q4_verify_tokens_sampled) at position p with the true continuation wrong at index k, for every k in 0 .. D (D: all
    right), each on rows ingested afresh by passes"""
    L = q4.lib()
    R = want["R"]
    q4.set_pass_context(S)
    t = q4.Transformer(path, pass_13b=True, **kw)
    try:
        if sampled:
            t.set_speculative(draft=7, ngram=3, min=1, sampled=True)
        for k in range(D + 1):
            before = L.q4_prompt_passes()
            if sampled:
                _set_rng(t, kw["seed"])                                   # (the loop draws and discards the prompt positions' coins)
            t.generate_ids(_LONG[:p + 1], p)
            assert t.pos() == p and L.q4_prompt_passes() - before == len(_passes(p + 1, p, S, t.config.seq_len))
            if D + 1 < MIN:            # fewer rows than this shape's minimum: refused, nothing runs
                assert not t.verify_covers(p, D) and t.verify([int(x) for x in R[p + 1:p + 1 + D]]) is None and t.pos() == p
                assert not t.verify_covers(p, MIN - 2) and t.verify_covers(p, MIN - 1)
                break
            assert t.verify_covers_sampled(p, D) if sampled else t.verify_covers(p, D)
            if poison is not None:
                cp.poison(q4, t, p, poison)
            drafts = [int(x) for x in R[p + 1:p + 1 + D]]
            if k < D:
                drafts[k] = (drafts[k] + 1) % vocab if sampled else _wrong(drafts[k])
            stats = t.spec_stats()
            emitted, acc = t.verify_sampled(drafts) if sampled else t.verify(drafts)
            what = "position %d, %d drafts, first wrong %d" % (p, D, k)
            assert acc == k and emitted.tolist() == R[p + 1:p + k + 2], what
            assert t.pos() == p + k + 1 and [t.token(i) for i in range(p + k + 2)] == R[:p + k + 2], what
            assert t.spec_stats() == (stats[0] + 1, stats[1] + D, stats[2] + k), what
            assert np.array_equal(t.logits().view(np.uint16), want["logits"][k]), what + ": logits behind the pass"
            if sampled:
                assert tsg._rng_state(t) == want["rng"][k], what + ": rng_state"
            gk, gv = cp.read_rows(q4, t, 0, p + k + 1)
            for name, g, w in (("K", gk, want["k"]), ("V", gv, want["v"])):
                bad = np.argwhere((g != w[:, :p + k + 1]).any(axis=2))
                assert bad.size == 0, "%s: %s rows differ, first (layer, position) %s" % (what, name, [tuple(int(i) for i in x) for x in bad[:8]])
            if poison is not None:
                cp.assert_untouched(q4, t, p + D + 1, poison, what)
            q4.check(L.q4_handoff_status(t.state))
    finally:
        q4.set_pass_context(256)
        t.close()


_STEPWISE = {}


@pytest.mark.parametrize("D", [1, 4, 7])
@pytest.mark.parametrize("p", [30, 300, 600, 1100, 2100])
def test_verify_tokens(q4, models, p, D):
    """D drafts at position p, the first wrong one at every index 0 .. D - 1 and all right: tokens, n_accepted, the position, the rows below the new
    position and the logits against the stepwise run (computed once per position). One draft is two rows, below this shape's minimum of four: the
    probe says no and q4_verify_tokens refuses"""
    if p not in _STEPWISE:
        _STEPWISE[p] = _stepwise(q4, models(NAME), p)
    _verify_all_indices(q4, models(NAME), p, _STEPWISE[p], D=D)


# ---- 5. under the sampler, at Llama-2's vocabulary -----------------------------------------------------------------------------------------------------------
SAMPLED = dict(temperature=0.5, topp=0.6, seed=7)


@pytest.mark.parametrize("p", [30, 200])
def test_verify_tokens_sampled(q4, models, p):
    """k5120_cls (vocabulary 32000: the step's classifier runs as strips, ten pieces per row) at -t 0.5 -p 0.6, four drafts, every first-wrong index:
    tokens, rows, the probabilities a sampled step leaves in RunState::logits, rng_state"""
    want = _stepwise_sampled(q4, models(CLS), p, 4, **SAMPLED)
    _verify_all_indices(q4, models(CLS), p, want, D=4, sampled=True, vocab=32000, **SAMPLED)


def test_verify_tokens_greedy_at_vocabulary_32000(q4, models):
    _verify_all_indices(q4, models(CLS), 30, _stepwise(q4, models(CLS), 30, D=4), D=4)


@pytest.mark.parametrize("n", [1, 2, 3, 8])
def test_classifier_rows_at_dim_5120(q4, n):
    """q4_verify_classifier at dim 5120 row by row against q4_rmsnorm + q4_matmul_f16 -- at a ragged strips split (16600 rows over the CUs) and at 504
    rows (the plain fp16 GEMV); a zero row and a row of large values among them"""
    L = q4.lib()
    dim = 5120
    r = np.random.default_rng(3)
    for vocab in (16600, 504):
        w = (r.standard_normal((vocab, dim), dtype=np.float32) * 0.02).astype(np.float16)
        dw = q4.DevBuf(w)
        rms = q4.DevBuf((1.0 + 0.1 * r.uniform(-1, 1, dim)).astype(np.float16))
        x = r.standard_normal((8, dim), dtype=np.float32)
        x[1] = 0.0
        x[2] *= 30.0
        dx = q4.DevBuf(x.astype(np.float16))
        xn, lo, out = q4.DevBuf(nbytes=dim * 2), q4.DevBuf(nbytes=vocab * 2), q4.DevBuf(nbytes=8 * vocab * 2)
        q4.verify_classifier(out, dx, rms, dw, dim, vocab, n)
        got = out.get(np.uint16, 8 * vocab).reshape(8, vocab)
        for i in range(n):
            q4.check(L.q4_rmsnorm(xn.ptr, dx.ptr + i * dim * 2, rms.ptr, dim))
            q4.check(L.q4_matmul_f16(lo.ptr, xn.ptr, dw.ptr, dim, vocab, 1, 0, 0, 0, -1, 1.0))
            want = lo.get(np.uint16, vocab)
            bad = np.flatnonzero(got[i] != want)
            assert bad.size == 0, "vocabulary %d, row %d of %d: %d logits differ, first at %d" % (vocab, i, n, bad.size, bad[0])
        assert got[0].any() and (n < 2 or not got[1].any())


# ---- 6. the speculative loop ----------------------------------------------------------------------------------------------------------------------------------
_SPEC_OFF = {}


def _spec_off(q4, models, **kw):
    key = tuple(sorted(kw.items()))
    if key not in _SPEC_OFF:
        _SPEC_OFF[key] = tsg._run(q4, models(NAME), prompt=_prompt(N_SPEC), steps=300, groups=True, **kw)
        assert _SPEC_OFF[key]["stats"] == (0, 0, 0) and len(_SPEC_OFF[key]["tokens"]) == 301, "the off run meets an EOS: choose another seed"
    return _SPEC_OFF[key]


@pytest.mark.parametrize("kind", ["oracle", "wrong", "alternating"])
def test_speculative_loop(q4, models, kind):
    """a 17-token prompt to 300 steps with a scripted drafter -- the true continuation, always wrong, alternating: the run without speculation byte for
    byte, the counters of tests/spec_ref.py's replay"""
    off = _spec_off(q4, models)
    R = off["tokens"]
    on = tsg._run(q4, models(NAME), prompt=_prompt(N_SPEC), steps=300, spec=dict(draft=7, ngram=3, min=1), drafter=tsg.DRAFTERS[kind](R), pass_13b=True)
    tsg._assert_same(off, on, "%s drafter" % kind)
    want, passes = spec_ref.replay(R, N_SPEC, 300, _at_least(tsg.DRAFTERS[kind](R)), 7, lambda pos: off["groups"][pos])
    assert all(n >= MIN - 1 for _, n, _ in passes)
    print("%s: passes, drafted, accepted = %s (expected %s)" % (kind, on["stats"], want))
    assert on["stats"] == want and want[0] >= 10
    assert want[1] == want[2] if kind == "oracle" else want[2] == 0 if kind == "wrong" else 0 < want[2] < want[1]


@pytest.mark.parametrize("kind", ["oracle", "wrong", "alternating"])
def test_speculative_loop_sampled(q4, models, kind):
    off = _spec_off(q4, models, **SAMPLED)
    R = off["tokens"]
    on = tsg._run(q4, models(NAME), prompt=_prompt(N_SPEC), steps=300, drafter=tsg.DRAFTERS[kind](R), pass_13b=True, speculative=dict(draft=4, sampled=True),
                  **SAMPLED)
    tsg._assert_same(off, on, "sampled, %s drafter" % kind)
    assert on["stats"][0] >= 10, on["stats"]
    assert on["stats"][2] == on["stats"][1] if kind == "oracle" else on["stats"][2] == 0 if kind == "wrong" else 0 < on["stats"][2] < on["stats"][1], on["stats"]


# ---- 7. with records ------------------------------------------------------------------------------------------------------------------------------------------
def test_score_ids_by_passes(q4, models):
    tokens = _prompt(251, seed=9)
    res = {}
    for on in (False, True):
        t = q4.Transformer(models(NAME), logprobs=5, pass_logprobs=on, pass_13b=on)
        try:
            res[on] = _score(q4, t, tokens, 5)
        finally:
            t.close()
    off, on = res[False], res[True]
    assert off["passes"] == 0 and on["passes"] == 250 // T        # (the last two positions are below this shape's minimum: steps)
    assert on["lp"] == off["lp"] and np.isfinite(np.frombuffer(on["lp"], dtype=np.float32)).all()
    assert np.array_equal(on["logits"], off["logits"]) and on["pos"] == off["pos"] == 250
    assert on["records"] == off["records"]


def test_prompt_pass_with_records(q4, models):
    """a 64-token prompt and six steps with K = 5: records [0, pos), ring, rows and logits of the stepwise run"""
    off = _run(q4, models(NAME), _LONG[:64], on=False, ingest=0, logprobs=5)
    L = q4.lib()
    t = q4.Transformer(models(NAME), logprobs=5, pass_logprobs=True, pass_13b=True)
    s = q4.Transformer(models(NAME), logprobs=5)
    try:
        before = L.q4_prompt_passes()
        toks = t.generate_ids(_LONG[:64], 64 + GEN)[0].copy()
        assert L.q4_prompt_passes() - before == 8
        L.q4_set_prompt_ingest(0)
        s.generate_ids(_LONG[:64], 64 + GEN)
        L.q4_set_prompt_ingest(T)
        assert np.array_equal(toks, off["tokens"]) and t.pos() == s.pos() == off["pos"]
        assert _records(t, t.pos()) == _records(s, s.pos()), "records of a prompt by passes"
        assert np.array_equal(t.logits().view(np.uint16), off["logits"])
    finally:
        L.q4_set_prompt_ingest(T)
        t.close()
        s.close()


def test_verify_pass_with_records(q4, models):
    want = _stepwise(q4, models(NAME), 30, logprobs=5)
    R = want["R"]
    ref_t = q4.Transformer(models(NAME), logprobs=5)
    t = q4.Transformer(models(NAME), logprobs=5, pass_logprobs=True, pass_13b=True)
    try:
        q4.lib().q4_set_prompt_ingest(0)
        ref_t.generate_ids(R[:31], 34)
        q4.lib().q4_set_prompt_ingest(T)
        assert ref_t.pos() == 34
        t.generate_ids(_LONG[:31], 30)
        drafts = [int(x) for x in R[31:38]]
        drafts[3] = _wrong(drafts[3])
        assert t.verify_covers(30, 7)
        emitted, acc = t.verify(drafts)
        assert acc == 3 and emitted.tolist() == R[31:35] and t.pos() == 34
        assert _records(t, 34) == _records(ref_t, 34), "records [0, 34)"
        assert np.array_equal(t.logits().view(np.uint16), want["logits"][3])
    finally:
        q4.lib().q4_set_prompt_ingest(T)
        t.close()
        ref_t.close()


# ---- 8. one logit-stage case: the shared loop is shared --------------------------------------------------------------------------------------------------------
def test_logit_stages(q4, models):
    """top-k 40 and a repeat penalty under q4_set_pass_stages with the alternating drafter: the verify passes run the stages' row forms between this
    shape's classifier and the accept launch; the stepwise run's bytes"""
    kw = dict(sampling=dict(top_k=40, repeat_penalty=1.1, penalty_last_n=64))
    L = q4.lib()
    L.q4_set_prompt_ingest(0)
    try:
        off = tsg._run(q4, models(NAME), prompt=_prompt(N_SPEC), steps=120, **kw)
    finally:
        L.q4_set_prompt_ingest(T)
    R = off["tokens"]
    assert off["stats"] == (0, 0, 0) and len(R) == 121
    on = tsg._run(q4, models(NAME), prompt=_prompt(N_SPEC), steps=120, spec=dict(draft=7, ngram=3, min=1), drafter=tsg.DRAFTERS["alternating"](R), pass_13b=True,
                  pass_stages=True, **kw)
    tsg._assert_same(off, on, "top-k 40 + repeat penalty")
    assert on["stats"][0] >= 5 and 0 < on["stats"][2] < on["stats"][1], on["stats"]


# ---- 9. stale rows ----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", cp.PATTERNS)
@pytest.mark.parametrize("start,n", [(40, 100), (600, 660)])
def test_stale_rows_prompt_pass(q4, models, pattern, start, n):
    """every row from `start` up poisoned in front of prompt passes resumed there: the clean run's bytes, nothing written more than PROMPT_PASS_MAX rows
    above where the run ends"""
    prompt = _LONG[:n]
    off = _off(q4, models, n)
    on = _run(q4, models(NAME), prompt, bound=S, start=start, warm=prompt[:start + 1], poison=(pattern, start))
    assert on["passes"] == len(_passes(n, n + GEN, S, S, start=start)) > 0
    _assert_same(off, on, "%s from row %d" % (pattern, start), rng=False)


@pytest.mark.parametrize("pattern", cp.PATTERNS)
def test_stale_rows_verify_pass(q4, models, pattern):
    if 600 not in _STEPWISE:
        _STEPWISE[600] = _stepwise(q4, models(NAME), 600)
    _verify_all_indices(q4, models(NAME), 600, _STEPWISE[600], poison=pattern)


# ---- 10. hostile weights ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("trait", ["massive", "quant_edges"])
def test_hostile_weights(q4, models, trait):
    """massive residual channels, and pinned zero points / q == z groups / scales over two decades: the half slot's 0.f addend and the even / odd
    placement are where a restated sum parts from the original, and such values show it where Gaussian weights hide it. 17 prompt tokens by passes, and
    q4_verify_tokens at position 30 at every first-wrong index."""
    path = models(NAME, trait)
    off = _off(q4, models, 2 * T + 1, trait=trait)
    assert cp.finite(off["k"]) and cp.finite(off["v"]) and cp.finite(off["logits"]), trait
    on = _run(q4, path, _LONG[:2 * T + 1])
    assert on["passes"] == 2
    _assert_same(off, on, "%s, 17 prompt tokens" % trait)
    want = _stepwise(q4, path, 30)
    assert all(cp.finite(x) for x in want["logits"])
    _verify_all_indices(q4, path, 30, want)


def test_against_the_restatement_and_the_double_forward(q4, orc, models, observed):
    """tests/test_pass_hostile_gpu.py's (b) at this width, on the massive-channel checkpoint: SEQ as a 14-token prompt (a pass of eight, one of five, the
    generating step). The logits behind position 13 and the K / V rows of both layers at all 14 positions against oracle.Model under that file's
    default bounds, the logits against the unrounded double forward under its bracket; the same run by steps beside it must be the pass's bytes."""
    path, key = models(NAME, "massive"), "%s/massive" % NAME
    ref_logits, (rk, rv), _ = hostile_ref.restatement(orc, path, (NAME, "massive", SEED), SEQ, 1)
    f64 = hostile_ref.f64_last(orc, path, (NAME, "massive", SEED), SEQ)
    on = _run(q4, path, SEQ, steps=len(SEQ))
    off = _run(q4, path, SEQ, steps=len(SEQ), on=False, ingest=0)
    assert on["passes"] == 2 == len(_passes(len(SEQ), len(SEQ), 256, S)) and off["passes"] == 0
    _assert_same(off, on, key + ", SEQ as a prompt")
    last = len(SEQ) - 1
    k, v = on["k"], on["v"]
    assert k.shape[1] == len(SEQ)
    f = lambda u: u.view(np.float16)
    err = np.array([max(float(_rel(f(k[:, i]), rk[:, i]).max()), float(_rel(f(v[:, i]), rv[:, i]).max())) for i in range(len(SEQ))])
    got = on["logits"].view(np.float16)
    e = float(_rel(got, ref_logits[last]).max())
    eg, er = float(_rel(got, f64).max()), float(_rel(ref_logits[last], f64).max())
    rg, rr = _rms(got, f64), _rms(ref_logits[last], f64)
    observed.setdefault("pass_13b_vs_restatement", {})[key] = dict(logits=e, kv=float(err.max()), f64_max_gpu=eg, f64_max_restatement=er)
    print("%s: logits %.3g (bound %g), K / V rows %.3g (bound %g); f64 max %.3g vs %.3g, rms %.3g vs %.3g" % (key, e, DEFAULT_BOUND, err.max(), DEFAULT_KV_BOUND, eg, er, rg, rr))
    assert e <= DEFAULT_BOUND, "%s: max rel logit err %g behind position %d" % (key, e, last)
    assert err.max() <= DEFAULT_KV_BOUND, "%s: K / V rows at position %d: %g" % (key, int(err.argmax()), err.max())
    assert eg <= 2.0 * er + 1e-3, "%s: GPU %g vs restatement %g from the unrounded forward" % (key, eg, er)
    assert rg <= 1.5 * rr + 1e-4, "%s: rms GPU %g vs restatement %g from the unrounded forward" % (key, rg, rr)


# ---- 11. two models -------------------------------------------------------------------------------------------------------------------------------------------------
def test_two_models_alternate(q4, models):
    """a pass_long (4096-wide) and a k5120_pair Transformer alternate generations with passes: each keeps its own scratch rows and its own bytes"""
    L = q4.lib()
    pa, pb = _LONG[:41], _prompt(57, seed=21)
    fresh = {(name, len(p)): _run(q4, models(name), p) for name in (WIDE7B, NAME) for p in (pa, pb)}
    ta, tb = q4.Transformer(models(WIDE7B)), q4.Transformer(models(NAME), pass_13b=True)
    try:
        for p in (pa, pb, pa):
            for name, t in ((WIDE7B, ta), (NAME, tb)):
                before = L.q4_prompt_passes()
                toks = t.generate_ids(p, len(p) + GEN)[0].copy()
                want = fresh[name, len(p)]
                assert L.q4_prompt_passes() - before == want["passes"] == (_expected_passes(len(p)) if name == WIDE7B else len(_passes(len(p), len(p) + GEN, 256, S)))
                k, v = cp.read_rows(q4, t, 0, t.pos())
                got = dict(tokens=toks, pos=t.pos(), k=k, v=v, logits=t.logits().view(np.uint16).copy(), rng=want["rng"])
                _assert_same(want, got, "%s, %d prompt tokens, alternating" % (name, len(p)))
                q4.check(L.q4_handoff_status(t.state))
    finally:
        ta.close()
        tb.close()
    _assert_same(_off(q4, models, 41), fresh[NAME, 41], "k5120_pair against the steps")


# ---- 12. not admitted, the switch on --------------------------------------------------------------------------------------------------------------------------------
NOT_ADMITTED = {
    "fp8 with pass_kv8": (NAME, None, dict(kv="fp8", pass_kv8=True)),
    "hidden 1408": ("head128_k5120", None, {}),
    "grouped-query": (NAME, "gqa", dict(pass_gqa=True)),
}


@pytest.mark.parametrize("case", sorted(NOT_ADMITTED))
def test_not_admitted(q4, models, case):
    name, trait, kw = NOT_ADMITTED[case]
    prompt = _LONG[:40]
    spec = dict(draft=4, ngram=3, min=1)
    on = _run(q4, models(name, trait), prompt, steps=100, bound=S, spec=spec, drafter=lambda ring, room: [5] * room, **kw)
    off = _run(q4, models(name, trait), prompt, steps=100, on=False, ingest=0, **kw)
    assert on["passes"] == 0 and on["stats"] == (0, 0, 0) and not any(on["covers"]), (case, on["passes"], on["stats"], on["covers"])
    _assert_same(off, on, case)


def test_a_4096_wide_model_is_unchanged(q4, models):
    """pass_long with the switch on: the pass counts and the bytes it has with the switch off"""
    prompt = _LONG[:140]
    a = _run(q4, models(WIDE7B), prompt, on=False)
    b = _run(q4, models(WIDE7B), prompt, on=True)
    assert a["passes"] == b["passes"] == _expected_passes(140) and a["covers"] == b["covers"]
    _assert_same(a, b, "pass_long, switch on against off")


def test_step_form_knobs_keep_the_steps():
    """q4_set_half_tail, q4_set_ksplit and the GEMV form exist in the profiling build only: tests/pass_13b_prof_cases.py runs against it in a process of
    its own"""
    env = dict(os.environ, Q4_PROFILING_BUILD="1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "pass_13b_prof_cases.py"), "-x", "-q", "-m", "gpu",
                        "-p", "no:cacheprovider"], env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert " passed" in r.stdout
