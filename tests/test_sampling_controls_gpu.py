"""Sampling controls inside the decode step (csrc/q4_logit_process.hip, q4_sampler_set_controls / _set_logit_bias, q4_process_logits): the launch on
crafted logits against the numpy float32 reference (tests/sampling_controls_ref.py) BIT FOR BIT, min-p's kept set, the sampler's tokens on processed
logits, and the launch inside the step in every graph form against a ground truth rebuilt from a controls-off model's raw logits."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import logprobs_ref
import sampling_controls_ref as ref
import teacher_forced
from conftest import GOLDEN, ROOT
from llama_cu_awq_amd import synth
from test_logprobs_gpu import HIGH, _distributions

pytestmark = pytest.mark.gpu

ERR_ARG = 5
PENALTIES = dict(repeat_penalty=1.3, presence_penalty=0.5, frequency_penalty=0.25)
NINF = float("-inf")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float16).view(np.uint16)


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. the op against the reference
def _windows(rng, n, lo=0):
    """(name, ring, pos, last_n): empty, 1, 64 and 1024 entries; few distinct tokens (heavy repeats) and ids outside [0, n). lo: the least valid id"""
    out = []
    for name, last_n, pos in (("empty", 0, 5), ("1", 1, 0), ("64", 64, 100), ("1024", 1024, 1500)):
        ring = (lo + rng.integers(0, min(n - lo, 50), pos + 4)).astype(np.int32)
        if pos > 8:
            ring[rng.choice(pos + 1, size=(pos + 1) // 8, replace=False)] = rng.choice([-5, n, n + 7, 2 ** 31 - 1, -2 ** 31], size=(pos + 1) // 8)
            ring[pos - 3:pos + 1] = ring[pos]                    # the newest token four times over
        out.append((name, ring, pos, last_n))
    return out


def _biases(rng, n, lo=0):
    """{id: bias} of 0, 1 and 256 entries (as many as the vocabulary has), -inf among them, ids that are in the windows among them. lo: the least id"""
    out = [{}]
    for count in (1, 256):
        count = min(count, n)
        ids = set(range(lo, lo + min(count // 2, n - lo))) | set(lo + int(i) for i in rng.choice(n - lo, size=count, replace=False))
        ids = (sorted(ids)[:count // 2] + sorted(ids)[-(count - count // 2):] if lo else sorted(ids)[:count]) if count > 1 else [lo + int(rng.integers(min(n - lo, 50)))]
        b = {i: float(np.float32(rng.standard_normal() * 3.0)) for i in ids}
        if count > 1:
            for i in ids[::5]:
                b[i] = NINF
            b[ids[1]] = 65504.0                                  # onto the clamp
        out.append(b)
    return out


def _process(q4, x, ring=None, pos=None, logit_bias=None, **kw):
    dl = q4.DevBuf(x)
    dr = q4.DevBuf(ring) if ring is not None else None
    dp = q4.DevBuf(np.array([pos], dtype=np.int32)) if pos is not None else None
    q4.process_logits(dl, x.shape[0], logit_bias=logit_bias, tokens=dr, pos=dp, **kw)
    q4.synchronize()
    return dl.get(np.float16, x.shape[0])


def _with_nan(rng, n, lo=0):
    """lo > 0: as _distributions -- the entries below id lo 40 down, the NaN at a fixed id above it"""
    x = (rng.standard_normal(n) * 2.0).astype(np.float16)
    if lo:
        x[:lo] = (x[:lo].astype(np.float32) - 40.0).astype(np.float16)
        x[100003] = np.nan
    else:
        x[int(rng.integers(n))] = np.nan
    return x


@pytest.mark.parametrize("n", [1, 8, 20, 1000, 1027, 32000, 32768, 32776, 40000, 128256, 128259])
def test_op_matches_the_reference_bit_for_bit(q4, n):
    """(128256 / 128259: beyond 16 bits of token id. There every penalised id, every biased id, the maximum and the entries a top-k keeps sit at ids >= 65536,
    some beyond 98304: asserted on the reference's answer.)"""
    rng = np.random.default_rng(2000 + n)
    lo = HIGH if n > HIGH else 0
    windows, biases = _windows(rng, n, lo), _biases(rng, n, lo)
    if lo:
        assert all(min(b) >= lo for b in biases if b) and max(max(b) for b in biases if b) > 98304
        assert all(((r >= lo) | (r < 0)).all() for _, r, _, _ in windows)
    combos = [(w, b) for w in range(len(windows)) for b in range(len(biases))]
    case = highest = 0
    seen = set()
    for k in (0, 1, 40, n):
        if k > n:
            continue
        dists = [(name, x) for name, x, _ in _distributions(rng, n, k, lo)] + [("one NaN", _with_nan(rng, n, lo))]
        for name, x in dists:
            wi, bi = combos[case % len(combos)]                  # every (window, bias list) pair comes round for every n
            case += 1
            seen.add((wi, bi))
            wname, ring, pos, last_n = windows[wi]
            kw = dict(top_k=k, penalty_last_n=last_n, **PENALTIES)
            what = "n %d k %d %s, window %s, %d biases" % (n, k, name, wname, len(biases[bi]))
            got = _process(q4, x, ring, pos, biases[bi], **kw)
            want = ref.process(x, tokens=ring, pos=pos, logit_bias=biases[bi], **kw)
            bad = np.nonzero(_bits(got) != _bits(want))[0]
            assert bad.size == 0, "%s: %d entries differ, first %d: got %04x, reference %04x (input %04x)" % (
                what, bad.size, bad[0], _bits(got)[bad[0]], _bits(want)[bad[0]], _bits(x)[bad[0]])
            assert got.size == n
            if lo:                                               # on the reference's output: the maximum (its lowest index) and what a top-k keeps, beyond 16 bits
                w32 = want.astype(np.float32)
                with np.errstate(invalid="ignore"):
                    assert int(np.flatnonzero(w32 == np.nanmax(w32)).min()) >= lo, what
                if 0 < k < n:
                    kept = np.flatnonzero(~np.isneginf(w32))
                    assert kept.size >= 1 and kept.min() >= lo, (what, kept[:4])
                    highest = max(highest, int(kept.max()))
            again = _process(q4, x, ring, pos, biases[bi], **kw)
            assert again.tobytes() == got.tobytes(), what + ": a second launch gave other bytes"
    assert seen == set(combos)
    assert not lo or highest > 98304, highest


def test_op_window_shorter_than_last_n_and_no_ring(q4):
    """the window stops at ring index 0; without a ring (NULL) there is no window; top_k alone reads none"""
    rng = np.random.default_rng(5)
    x = (rng.standard_normal(1000) * 2.0).astype(np.float16)
    ring = rng.integers(0, 30, 16).astype(np.int32)
    kw = dict(penalty_last_n=64, **PENALTIES)
    assert _process(q4, x, ring, 9, **kw).tobytes() == ref.process(x, tokens=ring, pos=9, **kw).tobytes()
    assert _process(q4, x, None, None, top_k=40, **kw).tobytes() == ref.process(x, top_k=40).tobytes()
    assert _process(q4, x, ring, 9, top_k=7).tobytes() == ref.process(x, top_k=7).tobytes()
    L = q4.lib()
    d = q4.DevBuf(x)
    c = q4.SamplingControls(top_k=1001)
    assert L.q4_process_logits(d.ptr, 1000, C.byref(c), None, None, 0, None, None) == ERR_ARG


@pytest.mark.parametrize("n", [1000, 32000, 40000])
def test_min_p_keeps_the_reference_set(q4, n):
    """The threshold is a logf: the test first checks ON THE CPU that none of its inputs lies within 2^-20 |ln min_p| of it (ln in float64), so a
    last-bit difference between two logf cannot move an entry; then the kept set must be the reference's exactly (and so must every byte)."""
    rng = np.random.default_rng(3000 + n)
    ring = rng.integers(0, 40, 80).astype(np.int32)
    cases = 0
    for min_p in (0.02, 0.05, 0.3, 0.9):
        for scale in (1.0, 4.0):
            x = (rng.standard_normal(n) * scale).astype(np.float16)
            for kw in (dict(), dict(top_k=40), dict(top_k=40, penalty_last_n=64, **PENALTIES)):
                extra = dict(tokens=ring, pos=70, logit_bias={int(np.argmax(x)): NINF}) if "penalty_last_n" in kw else {}
                margin = ref.min_p_margin(x, min_p, **kw, **extra)
                assert margin > 2.0 ** -20, "an input within 2^-20 of the threshold: choose another seed (min_p %g, margin %g)" % (min_p, margin)
                got = _process(q4, x, extra.get("tokens"), extra.get("pos"), extra.get("logit_bias"), min_p=min_p, **kw)
                want = ref.process(x, min_p=min_p, **kw, **extra)
                assert np.array_equal(np.isneginf(got), np.isneginf(want)), "min_p %g scale %g %s: kept %d, reference %d" % (
                    min_p, scale, kw, (~np.isneginf(got)).sum(), (~np.isneginf(want)).sum())
                assert got.tobytes() == want.tobytes()
                assert (~np.isneginf(got)).sum() >= 1
                cases += 1
    assert cases == 24


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. the sampler's tokens on processed logits
@pytest.fixture(scope="module")
def paths(tmp_path_factory):
    d = tmp_path_factory.mktemp("sc")
    out = {}
    for name in ("small", "v32k", "v40k"):
        out[name] = str(d / (name + ".bin"))
        synth.write_model(out[name], name, seed=7)
    return out


@pytest.mark.parametrize("name", ["small", "v32k"])
@pytest.mark.parametrize("temperature,topp", [(0.8, 0.9), (1.0, 0.0)])
def test_sampler_tokens_on_processed_logits(q4, orc, paths, name, temperature, topp):
    L = q4.lib()
    t = q4.Transformer(paths[name], temperature=temperature, topp=topp, seed=77)
    vocab = t.config.vocab_size
    rng = np.random.default_rng(vocab + int(10 * topp))
    state = C.c_ulonglong(77)
    ring = rng.integers(0, 60, 64).astype(np.int32)
    dr, dp = q4.DevBuf(ring), q4.DevBuf(np.array([50], dtype=np.int32))
    kw = dict(top_k=40, min_p=0.02, penalty_last_n=16, **PENALTIES)
    logits = q4.DevBuf(nbytes=2 * vocab)
    bad = []
    for trial in range(12):
        x = (rng.standard_normal(vocab) * (1.0 + trial % 3)).astype(np.float16)
        bias = {int(np.argmax(x)): NINF, 5: 2.0}
        t.reset([1])
        q4.check(L.q4_memcpy_h2d(t.state.contents.logits, x.ctypes.data, x.nbytes))
        ids, b = q4._bias_arrays(bias)
        c = q4.SamplingControls(**kw)
        q4.check(L.q4_process_logits(t.state.contents.logits, vocab, C.byref(c), ids.ctypes.data, b.ctypes.data, len(ids), dr.ptr, dp.ptr))
        q4.check(L.q4_sample(t.sampler, t.state, 1))
        q4.synchronize()
        coin = L.random_f32(C.byref(state))
        want = ref.process(x, tokens=ring, pos=50, logit_bias=bias, **kw)
        tok = orc.lib().orc_sample_topp(orc.f16_bits(want.copy()), vocab, temperature, topp, coin)
        if t.token(1) != tok:
            bad.append((trial, int(t.token(1)), tok, coin))
        assert t.token(1) != int(np.argmax(x))
    assert not bad, bad
    t.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. inside the step
PROMPT = [1, 5, 9]
SAMPLED = (0.8, 0.9)
SEED = 4242
STEPS = {"small": 300, "v32k": 32, "v40k": 32}                   # small: the bins 128 / 256, eight steps per replay; the others: their whole context


def _sampler(mode):
    return dict(temperature=SAMPLED[0], topp=SAMPLED[1], seed=SEED) if mode == "sampled" else dict(temperature=0.0)


def _controls(**over):
    c = dict(top_k=40, min_p=0.02, penalty_last_n=16, **PENALTIES)
    c.update(over)
    return c


def _stepwise(q4, t, prompt, steps):
    """the reference-shaped loop: one run_transformer call per step, synchronised, the next token read from the ring by the device"""
    t.reset(prompt)
    for pos in range(steps):
        t.run_transformer(pos >= len(prompt) - 1)
        q4.synchronize()
    return np.array([t.token(i) for i in range(steps + 1)], dtype=np.int32)


def _raw_logits(q4, path, tokens):
    return teacher_forced.raw_logits(q4, path, tokens)


def _predict(q4, orc, raw, tokens, n_prompt, controls, bias, mode, first_coin=0):
    return teacher_forced.predict(q4, orc, raw, tokens, n_prompt, controls, bias, mode, SEED, SAMPLED, first_coin)


@pytest.fixture(scope="module")
def runs(q4, orc, paths):
    """per (model, mode), once: the run that never called a setter, the controlled run (eight steps per replay), the controlled stepwise run,
    the raw logits of the controlled run's ring"""
    L = q4.lib()
    out = {}
    for name in ("small", "v32k", "v40k"):
        for mode in ("greedy", "sampled"):
            steps = STEPS[name]
            c0 = L.q4_graph_captures()
            t = q4.Transformer(paths[name], **_sampler(mode))
            plain = t.generate_ids(PROMPT, steps)[0].copy()
            r = dict(plain=plain, plain_logits=t.logits(), plain_captures=L.q4_graph_captures() - c0)
            t.close()
            bias = {int(plain[len(PROMPT)]): NINF}                # bans the unconstrained run's first generated token
            t = q4.Transformer(paths[name], sampling=_controls(), logit_bias=bias, **_sampler(mode))
            r["tokens"] = t.generate_ids(PROMPT, steps)[0].copy()
            r["logits"] = t.logits()
            t.close()
            t = q4.Transformer(paths[name], sampling=_controls(), logit_bias=bias, **_sampler(mode))
            r["stepwise"] = _stepwise(q4, t, PROMPT, steps)
            t.close()
            r["bias"] = bias
            r["raw"] = _raw_logits(q4, paths[name], r["tokens"]) if len(r["tokens"]) == steps + 1 else None
            out[(name, mode)] = r
    return out


CASES = [(n, m) for n in ("small", "v32k", "v40k") for m in ("greedy", "sampled")]


@pytest.mark.parametrize("name,mode", CASES)
def test_grouped_steps_equal_the_stepwise_loop(runs, name, mode):
    """(a) generate_ids (eight steps per replay, the bins 128 / 256 on `small`) against one run_transformer call per step"""
    r = runs[(name, mode)]
    assert len(r["tokens"]) == STEPS[name] + 1, "the run stopped at an EOS: pick another seed"
    assert np.array_equal(r["tokens"], r["stepwise"][:len(r["tokens"])]), "first difference at %d" % int(np.nonzero(r["tokens"] != r["stepwise"])[0][0])
    assert not np.array_equal(r["tokens"], r["plain"]), "the controls changed nothing"


@pytest.mark.parametrize("name,mode", CASES)
def test_tokens_are_what_the_reference_predicts(q4, orc, runs, name, mode):
    """(b) the controlled run's ring, rebuilt from a controls-off model's raw logits, the numpy reference and the restated sampler"""
    r = runs[(name, mode)]
    want = _predict(q4, orc, r["raw"], r["tokens"], len(PROMPT), _controls(), r["bias"], mode)
    bad = np.nonzero(want != r["tokens"])[0]
    assert bad.size == 0, "%s %s: %d tokens differ, first at ring index %d: %d, reference %d" % (name, mode, bad.size, bad[0], r["tokens"][bad[0]], want[bad[0]])
    if mode == "greedy":         # after a greedy generating step RunState::logits holds the PROCESSED logits
        last = len(r["tokens"]) - 2
        assert r["logits"].tobytes() == ref.process(r["raw"][last], tokens=r["tokens"], pos=last, logit_bias=r["bias"], **_controls()).tobytes()


@pytest.mark.parametrize("name", ["small", "v32k"])
def test_ban_and_top_k_one(q4, paths, runs, name):
    """(c) the banned token never appears; with top_k = 1 the sampled run is the greedy one"""
    for mode in ("greedy", "sampled"):
        r = runs[(name, mode)]
        banned = next(iter(r["bias"]))
        assert banned == r["plain"][len(PROMPT)] and banned not in r["tokens"][len(PROMPT):].tolist()
    bias = runs[(name, "greedy")]["bias"]
    got = {}
    for mode in ("greedy", "sampled"):
        t = q4.Transformer(paths[name], sampling=_controls(top_k=1), logit_bias=bias, **_sampler(mode))
        got[mode] = t.generate_ids(PROMPT, STEPS[name])[0].copy()
        t.close()
    assert np.array_equal(got["greedy"], got["sampled"])
    assert len(set(runs[(name, "sampled")]["tokens"][len(PROMPT):].tolist())) > 8


@pytest.mark.parametrize("mode", ["greedy", "sampled"])
def test_off_is_exactly_today(q4, paths, runs, mode):
    """(d) controls set and cleared again, or set to all-neutral values: tokens, the final logits' bytes and the graphs captured are those of a
    run that never called a setter"""
    L = q4.lib()
    r = runs[("small", mode)]
    for how in ("cleared", "neutral"):
        c0 = L.q4_graph_captures()
        t = q4.Transformer(paths["small"], **_sampler(mode))
        if how == "cleared":
            t.set_sampling(**_controls())
            t.set_logit_bias({7: -1.0})
            t.set_sampling()
            t.set_logit_bias(None)
        else:
            t.set_sampling(top_k=0, min_p=0.0, repeat_penalty=1.0, presence_penalty=0.0, frequency_penalty=0.0, penalty_last_n=64)
            t.set_logit_bias({})
        toks = t.generate_ids(PROMPT, STEPS["small"])[0].copy()
        logits = t.logits()
        t.close()
        assert np.array_equal(toks, r["plain"]), how
        assert logits.tobytes() == r["plain_logits"].tobytes(), how
        assert L.q4_graph_captures() - c0 == r["plain_captures"], how


def test_changing_the_controls_between_sequences(q4, orc, paths, runs):
    """(e) other controls and another bias for the second sequence on ONE model: the second sequence is what the reference predicts for the new
    values -- no graph is replayed with stale ones -- and nothing is captured again (the values are not part of a graph); switching them off and
    on again captures again"""
    L = q4.lib()
    r = runs[("small", "greedy")]
    steps = 60
    t = q4.Transformer(paths["small"], sampling=_controls(), logit_bias=r["bias"])
    first = t.generate_ids(PROMPT, steps)[0].copy()
    assert np.array_equal(first, r["tokens"][:steps + 1])
    c0 = L.q4_graph_captures()
    second_controls = _controls(top_k=5, repeat_penalty=1.7, penalty_last_n=64, min_p=0.0)
    second_bias = {int(first[len(PROMPT)]): NINF, int(first[len(PROMPT) + 1]): -4.0}
    t.set_sampling(**second_controls)
    t.set_logit_bias(second_bias)
    second = t.generate_ids(PROMPT, steps)[0].copy()
    assert L.q4_graph_captures() == c0, "changing a value captured graphs again"
    assert not np.array_equal(second, first)
    want = _predict(q4, orc, _raw_logits(q4, paths["small"], second), second, len(PROMPT), second_controls, second_bias, "greedy")
    assert np.array_equal(second, want)
    t.set_sampling()
    t.set_logit_bias(None)
    assert np.array_equal(t.generate_ids(PROMPT, steps)[0], r["plain"][:steps + 1])
    t.set_sampling(**_controls())
    t.set_logit_bias(r["bias"])
    assert np.array_equal(t.generate_ids(PROMPT, steps)[0], first)
    # a top_k or a bias id beyond the vocabulary is found by the first step that uses the sampler
    t.set_sampling(top_k=t.config.vocab_size + 1)
    t.reset(PROMPT)
    assert L.q4_run_transformer(1, C.byref(t.config), t.state, t.weights, 0, t.sampler) == ERR_ARG
    t.set_sampling(**_controls())
    t.set_logit_bias({t.config.vocab_size: 1.0})
    assert L.q4_run_transformer(1, C.byref(t.config), t.state, t.weights, 0, t.sampler) == ERR_ARG
    assert L.q4_run_transformer(0, C.byref(t.config), t.state, t.weights, 0, t.sampler) == 0      # a prompt step launches nothing
    t.close()


@pytest.mark.parametrize("mode", ["greedy", "sampled"])
def test_records_describe_the_raw_logits(q4, paths, runs, mode):
    """(f) with log-probability records on, the records are those of the model's raw logits -- the top order, and the log-probability of the token the
    step chose under them, greedy steps included (their token is no longer entry 0 of the raw order) -- and the tokens are unchanged"""
    r = runs[("small", mode)]
    steps, k = 40, 5
    t = q4.Transformer(paths["small"], sampling=_controls(), logit_bias=r["bias"], logprobs=k, **_sampler(mode))
    toks = t.generate_ids(PROMPT, steps)[0].copy()
    tlp, ids, top = t.logprobs(0, steps)
    t.close()
    assert np.array_equal(toks, r["tokens"][:steps + 1])
    for p in range(steps):
        x = r["raw"][p]
        rids, rlp = logprobs_ref.topk(x, k)
        assert np.array_equal(ids[p], rids), p
        assert logprobs_ref.within(top[p], rlp, logprobs_ref.bound(x, x[rids])), p
        tok = int(toks[p + 1])
        assert logprobs_ref.within([tlp[p]], [logprobs_ref.logprobs(x)[tok]], logprobs_ref.bound(x, x[tok])), p


def test_greedy_steps_are_not_screened_while_controls_are_on(q4, tmp_path):
    """(f) the screened classifier rewrites part of the logits only: with controls on no step uses it; cleared, the same model screens again"""
    path = str(tmp_path / "cls.bin")
    synth.write_model(path, "cls4096_ragged", seed=31)
    t = q4.Transformer(path, sampling=dict(top_k=40))
    t.generate_ids([1, 20, 300], 24)
    assert t.screen_candidates()[3] == 0
    t.set_sampling()
    t.generate_ids([1, 20, 300], 24)
    assert t.screen_candidates()[3] > 0, "the model does not screen at all: the check above shows nothing"
    t.close()


def test_cli_reads_the_environment_variable():
    """(g) Q4_SAMPLING through the built executable on the committed micro model"""
    exe = os.path.join(ROOT, "llama_cu_awq_amd", "bin", "llama2_q4")
    args = [exe, os.path.join(GOLDEN, "micro_model.bin"), "-n", "24", "-i", "Hello", "-t", "0.9", "-p", "0.95", "-s", "42", "-z", os.path.join(GOLDEN, "tokenizer.bin")]
    env = {k: v for k, v in os.environ.items() if k != "Q4_SAMPLING"}
    strip = lambda s: re.sub(r"achieved tok/s.*", "", s)
    run = lambda e: subprocess.run(args, capture_output=True, text=True, timeout=300, errors="replace", env=e)
    plain = run(env)
    on = run(dict(env, Q4_SAMPLING="top_k=3,repeat_penalty=1.5,last_n=16,presence=0.5"))
    again = run(dict(env, Q4_SAMPLING="top_k=3,repeat_penalty=1.5,last_n=16,presence=0.5"))
    assert plain.returncode == 0 and on.returncode == 0 and again.returncode == 0, (plain.stderr, on.stderr)
    assert strip(on.stdout) == strip(again.stdout)
    assert strip(on.stdout) != strip(plain.stdout)
    assert strip(run(dict(env, Q4_SAMPLING="")).stdout) == strip(plain.stdout)
    bad = run(dict(env, Q4_SAMPLING="top_k=many"))
    assert bad.returncode != 0 and "Q4_SAMPLING" in bad.stderr
