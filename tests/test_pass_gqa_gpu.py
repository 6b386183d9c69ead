"""Prompt and verify passes for the grouped-query 4096-wide shape (q4_set_pass_gqa; csrc/prompt_pass.hip, DESIGN.md 3.7 "Grouped-query shapes"): dim
4096, 32 query heads over 8 K / V heads, head 128, hidden 14336 -- Mistral-7B's and Llama-3-8B's layer, here twice with a context of 2304 (`gqa7b_pair`).
A pass restates the step's arithmetic, so "equal" always means BYTE-equal against the same library running per-token steps on a fresh Transformer: the
token ring, every K / V row (1024 halves) of both layers below the final position, the final logits, the position, the sampler's rng_state where there is
one. No tolerance anywhere.

The pieces a pass of this shape adds to Llama-2-7B's: the q/k/v launch with per-matrix widths (4096 / 1024 / 1024 columns in six-wave blocks), the
V-slice and the split-context attention with four query heads per K / V head, and the down projection's shared half slot (K = 14336: two k-parts of
224 = 3 x 64 + 32 units, the last slot's term a product and a sum on one half of the wave)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import cache_poison as cp
import hostile_models as hm
import pass_context_ref as ref
import spec_ref
import test_speculative_gpu as tsg
from conftest import ROOT
from llama_cu_awq_amd import synth
from test_pass_logprobs_gpu import _records, _score
from test_prompt_ingest_gpu import _expected_passes

pytestmark = pytest.mark.gpu

NAME = "gqa7b_pair"
MHA = "ffn_pair7b"
SEED = 11
T = 8
GEN = 6
S = 2304                  # gqa7b_pair's context, and the bound the long tests raise the setting to
AHEAD = 8                 # PROMPT_PASS_MAX: how far above the final position a pass may have written
N_LONG = 2200
N_SPEC = 17


@pytest.fixture(scope="module")
def models(tmp_path_factory):
    d = tmp_path_factory.mktemp("pass_gqa")
    made = {}

    def get(name, trait=None):
        if (name, trait) not in made:
            made[name, trait] = str(d / ("%s_%s.bin" % (name, trait)))
            if trait is None:
                synth.write_model(made[name, trait], name, seed=SEED)
            else:
                hm.write_hostile_model(made[name, trait], name, trait, seed=SEED)
        return made[name, trait]
    return get


def _prompt(n, seed=5):
    r = np.random.default_rng(seed)
    return [1] + [int(x) for x in r.integers(3, 512, size=n - 1)]       # no EOS (2) inside


_LONG = _prompt(N_LONG)


def _wrong(tok):
    w = (int(tok) + 1) % 512
    return w + 1 if w == 2 else w


def _run(q4, path, prompt, steps=None, gqa=True, ingest=T, graphs=1, bound=256, level=None, start=0, warm=None, poison=None, spec=None, drafter=None,
         verify=None, rows=True, **kw):
    """One generation on a fresh Transformer: dict(tokens, k, v (the rows below the final position), logits, pos, passes, stats, rng, covers).
    warm: a prompt generated first (start > 0 reuses its prefix). poison: (pattern, first row) written behind the warm run. verify: drafts for one
    q4_verify_tokens behind the generation. With poison, the rows from AHEAD above the final position must still hold it."""
    L = q4.lib()
    default = L.q4_get_prompt_ingest()
    timeouts = L.q4_handoff_timeouts()
    try:
        if level is not None:
            L.q4_set_fusion(level)
        L.q4_set_use_graphs(graphs)
        L.q4_set_prompt_ingest(ingest)
        q4.set_pass_context(bound)
        t = q4.Transformer(path, pass_gqa=gqa, **kw)
        try:
            assert t.pass_gqa() == bool(gqa)
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
            out = {"passes": L.q4_prompt_passes() - before, "covers": [int(L.q4_verify_covers(t.h, p, 4)) for p in (0, 40, 300, 600, 1100, 2100)]}
            if verify is not None:
                assert t.pos() == steps and t.verify_covers(steps, len(verify))
                emitted, acc = t.verify(verify)
                toks = np.array([t.token(i) for i in range(t.pos() + 1)], dtype=np.int32)
                out["accepted"], out["emitted"] = acc, emitted.tolist()
            q4.check(L.q4_handoff_status(t.state))
            assert L.q4_handoff_timeouts() == timeouts
            pos = t.pos()
            out.update(tokens=toks, pos=pos, logits=t.logits().view(np.uint16).copy(), stats=t.spec_stats(), rng=tsg._rng_state(t))
            if rows and kw.get("kv", "fp16") == "fp16":
                out["k"], out["v"] = cp.read_rows(q4, t, 0, pos)
                assert out["k"].shape[2] == t.config.dim * t.config.n_kv_heads // t.config.n_heads
            if poison is not None and pos + AHEAD < t.config.seq_len:
                cp.assert_untouched(q4, t, pos + AHEAD, poison[0], "final position %d" % pos)
        finally:
            t.close()
    finally:
        L.q4_set_prompt_ingest(default)
        L.q4_set_use_graphs(1)
        q4.set_pass_context(256)
        if level is not None:
            L.q4_set_fusion(q4.DEFAULT_FUSION)
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
        _OFF[key] = _run(q4, models(name, trait), _LONG[:n_prompt], gqa=False, ingest=0, graphs=graphs)
        assert _OFF[key]["passes"] == 0
    return _OFF[key]


# ---- 1. default off ---------------------------------------------------------------------------------------------------------------------------------------
def test_default_off(q4, models):
    """The switch off: no pass, q4_verify_covers 0 everywhere, the bytes of ingest off. On: the counter advances (without the feature it cannot), the
    probe reports the admission, and the bytes stay."""
    off = _off(q4, models, 2 * T + 1)
    plain = _run(q4, models(NAME), _LONG[:2 * T + 1], gqa=False, bound=S)
    assert plain["passes"] == 0 and plain["covers"] == [0] * 6
    _assert_same(off, plain, "switch off")
    on = _run(q4, models(NAME), _LONG[:2 * T + 1], bound=S)
    assert on["passes"] == _expected_passes(2 * T + 1) == 2
    assert on["covers"] == [1] * 6
    _assert_same(off, on, "switch on")
    t = q4.Transformer(models(NAME))
    try:
        assert not t.pass_gqa() and not t.verify_covers(30, 4)
        t.set_pass_gqa(True)
        assert t.pass_gqa() and t.verify_covers(30, 4) and t.verify_covers(248, 7) and not t.verify_covers(249, 7) and not t.verify_covers(300, 1)
        t.set_pass_gqa(False)
        assert not t.pass_gqa() and not t.verify_covers(30, 4)
    finally:
        t.close()


# ---- 2. prompt passes below 256 -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graphs", [1, 2])
@pytest.mark.parametrize("n_prompt", [2, 3, T, T + 1, 2 * T + 1, 130, 140])
def test_prompt_passes_below_256(q4, models, n_prompt, graphs):
    off = _off(q4, models, n_prompt, graphs)
    on = _run(q4, models(NAME), _LONG[:n_prompt], graphs=graphs)
    assert on["passes"] == _expected_passes(n_prompt)
    _assert_same(off, on, "%d prompt tokens, graphs %d" % (n_prompt, graphs))


def test_smaller_passes(q4, models):
    off = _off(q4, models, 2 * T + 1)
    on = _run(q4, models(NAME), _LONG[:2 * T + 1], ingest=3)
    assert on["passes"] == 16 // 3
    _assert_same(off, on, "passes of three")


# ---- 3. beyond 256 ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graphs", [1, 2, 0])
def test_long_prompt(q4, models, graphs):
    """2200 prompt tokens and six generated steps with the bound at the context: chunks of 64 / 128 / 256 and the eighteen-chunk last bin"""
    off = _off(q4, models, N_LONG, graphs)
    on = _run(q4, models(NAME), _LONG, graphs=graphs, bound=S)
    want = len(ref.prompt_passes(N_LONG, N_LONG + GEN, S, S, mode=graphs))
    print("graphs %d: prompt passes %d (expected %d)" % (graphs, on["passes"], want))
    assert on["passes"] == want and (graphs != 1 or want == 275)
    _assert_same(off, on, "2200 prompt tokens, graphs %d" % graphs)


@pytest.mark.parametrize("end", [255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049])
def test_prompt_ends(q4, models, end):
    """prompts whose last prompt-only position is `end`"""
    n = end + 2
    off = _off(q4, models, n)
    on = _run(q4, models(NAME), _LONG[:n], bound=S)
    assert on["passes"] == len(ref.prompt_passes(n, n + GEN, S, S))
    _assert_same(off, on, "last prompt-only position %d" % end)


def test_intermediate_bound(q4, models):
    off = _off(q4, models, 900)
    on = _run(q4, models(NAME), _LONG[:900], bound=600)
    assert on["passes"] == len(ref.prompt_passes(900, 900 + GEN, 600, S)) == 75
    _assert_same(off, on, "bound 600")


@pytest.mark.parametrize("start,n", [(5, 140), (300, 700)])
def test_resumed(q4, models, start, n):
    """generate_ids_from over a warm prefix (itself ingested by passes): the full per-token run's bytes"""
    prompt = _LONG[:n]
    off = _off(q4, models, n)
    on = _run(q4, models(NAME), prompt, bound=S, start=start, warm=prompt[:start] + _prompt(40, seed=9)[1:])
    assert on["passes"] == len(ref.prompt_passes(n, n + GEN, S, S, start=start))
    _assert_same(off, on, "resumed at %d" % start, rng=False)         # (the warm generation has drawn coins of its own)


# ---- 4. verify passes ---------------------------------------------------------------------------------------------------------------------------------------
def _stepwise(q4, path, p, D=7, **kw):
    """P[:p + 1] stepped to position p, then D + 1 generating steps one by one: the true continuation R[p + 1 .. p + D + 1], and behind step i the logits
    and the position; the rows [0, p + D + 1) at the end"""
    L = q4.lib()
    L.q4_set_prompt_ingest(0)
    t = q4.Transformer(path, **kw)
    try:
        t.generate_ids(_LONG[:p + 1], p)
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


def _verify_all_indices(q4, path, p, want, poison=None, D=7, **kw):
    """q4_verify_tokens at position p with the true continuation wrong at index k, for every k in 0 .. D, each on rows ingested afresh by passes"""
    L = q4.lib()
    R = want["R"]
    q4.set_pass_context(S)
    t = q4.Transformer(path, pass_gqa=True, **kw)
    try:
        for k in range(D + 1):
            before = L.q4_prompt_passes()
            t.generate_ids(_LONG[:p + 1], p)
            assert t.pos() == p and L.q4_prompt_passes() - before == len(ref.prompt_passes(p + 1, p, S, S))
            assert t.verify_covers(p, D)
            if poison is not None:
                cp.poison(q4, t, p, poison)
            drafts = [int(x) for x in R[p + 1:p + 1 + D]]
            if k < D:
                drafts[k] = _wrong(drafts[k])
            stats = t.spec_stats()
            emitted, acc = t.verify(drafts)
            what = "position %d, first wrong %d" % (p, k)
            assert acc == k and emitted.tolist() == R[p + 1:p + k + 2], what
            assert t.pos() == p + k + 1 and [t.token(i) for i in range(p + k + 2)] == R[:p + k + 2], what
            assert t.spec_stats() == (stats[0] + 1, stats[1] + D, stats[2] + k), what
            assert np.array_equal(t.logits().view(np.uint16), want["logits"][k]), what + ": logits behind the pass"
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


@pytest.mark.parametrize("p", [30, 120, 200, 300, 600, 1100, 2100])
def test_verify_tokens(q4, models, p):
    """seven drafts at position p (120: the pass ends at 127, the last position of bin 128), every first-wrong index 0 .. 7: tokens, n_accepted, the
    position, the rows below the new position and the logits against the stepwise run"""
    _verify_all_indices(q4, models(NAME), p, _stepwise(q4, models(NAME), p))


_SPEC_OFF = {}


def _spec_off(q4, models, **kw):
    key = tuple(sorted(kw.items()))
    if key not in _SPEC_OFF:
        _SPEC_OFF[key] = tsg._run(q4, models(NAME), prompt=_prompt(N_SPEC), steps=300, groups=True, **kw)
        assert _SPEC_OFF[key]["stats"] == (0, 0, 0) and len(_SPEC_OFF[key]["tokens"]) == 301, "the off run meets an EOS: choose another seed"
    return _SPEC_OFF[key]


@pytest.mark.parametrize("kind", ["oracle", "wrong"])
def test_speculative_loop(q4, models, kind):
    """a 17-token prompt to 300 steps with a forced drafter -- the true continuation, or always wrong: the run without speculation byte for byte, the
    counters of tests/spec_ref.py's replay"""
    off = _spec_off(q4, models)
    R = off["tokens"]
    on = tsg._run(q4, models(NAME), prompt=_prompt(N_SPEC), steps=300, spec=dict(draft=7, ngram=3, min=1), drafter=tsg.DRAFTERS[kind](R), pass_gqa=True)
    tsg._assert_same(off, on, "%s drafter" % kind)
    want, passes = spec_ref.replay(R, N_SPEC, 300, tsg.DRAFTERS[kind](R), 7, lambda pos: off["groups"][pos])
    print("%s: passes, drafted, accepted = %s (expected %s)" % (kind, on["stats"], want))
    assert on["stats"] == want and want[0] >= 10
    assert want[1] == want[2] if kind == "oracle" else want[2] == 0


# ---- 5. under the sampler -------------------------------------------------------------------------------------------------------------------------------------
def test_sampled(q4, models):
    """vocabulary 512 is admitted under the temperature / top-p sampler: tokens, rows, logits and rng_state of the run without speculation"""
    kw = dict(temperature=0.5, topp=0.6, seed=7)
    off = _spec_off(q4, models, **kw)
    R = off["tokens"]
    on = tsg._run(q4, models(NAME), prompt=_prompt(N_SPEC), steps=300, drafter=tsg.DRAFTERS["alternating"](R), pass_gqa=True,
                  speculative=dict(draft=4, sampled=True), **kw)
    tsg._assert_same(off, on, "sampled, alternating drafter")
    assert on["stats"][0] >= 10 and 0 < on["stats"][2] < on["stats"][1], on["stats"]


# ---- 6. with records --------------------------------------------------------------------------------------------------------------------------------------------
def test_score_ids_by_passes(q4, models):
    tokens = _prompt(251, seed=9)
    res = {}
    for on in (False, True):
        t = q4.Transformer(models(NAME), logprobs=5, pass_logprobs=on, pass_gqa=on)
        try:
            res[on] = _score(q4, t, tokens, 5)
        finally:
            t.close()
    off, on = res[False], res[True]
    assert off["passes"] == 0 and on["passes"] == 250 // T + 1
    assert on["lp"] == off["lp"] and np.isfinite(np.frombuffer(on["lp"], dtype=np.float32)).all()
    assert np.array_equal(on["logits"], off["logits"]) and on["pos"] == off["pos"] == 250
    assert on["records"] == off["records"]


def test_verify_pass_with_records(q4, models):
    want = _stepwise(q4, models(NAME), 30, logprobs=5)
    R = want["R"]
    ref_t = q4.Transformer(models(NAME), logprobs=5)
    t = q4.Transformer(models(NAME), logprobs=5, pass_logprobs=True, pass_gqa=True)
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


# ---- 7. stale rows ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", cp.PATTERNS)
@pytest.mark.parametrize("start,n", [(40, 100), (600, 660)])
def test_stale_rows_prompt_pass(q4, models, pattern, start, n):
    """every row from `start` up poisoned in front of prompt passes resumed there: the clean run's bytes, nothing written more than PROMPT_PASS_MAX rows
    above where the run ends"""
    prompt = _LONG[:n]
    off = _off(q4, models, n)
    on = _run(q4, models(NAME), prompt, bound=S, start=start, warm=prompt[:start + 1], poison=(pattern, start))
    assert on["passes"] == len(ref.prompt_passes(n, n + GEN, S, S, start=start)) > 0
    _assert_same(off, on, "%s from row %d" % (pattern, start), rng=False)


@pytest.mark.parametrize("pattern", cp.PATTERNS)
@pytest.mark.parametrize("p", [40, 600])
def test_stale_rows_verify_pass(q4, models, pattern, p):
    _verify_all_indices(q4, models(NAME), p, _stepwise(q4, models(NAME), p), poison=pattern)


def test_stale_rows_control(q4, models):
    """a NaN V row BELOW the position shows in what the prompt passes behind it leave (layer 1's rows of the first position they compute): the poison
    reaches the pass's attention through that pointer and layout"""
    L = q4.lib()
    q4.set_pass_context(S)
    t = q4.Transformer(models(NAME), pass_gqa=True)
    try:
        for p in (40, 600):
            t.generate_ids(_LONG[:p + 1], p)
            n_layers, seq_len, kv_dim = cp._shape(t)
            row = cp.pattern_row("nan", kv_dim)
            q4.check(L.q4_stream_synchronize())
            q4.check(L.q4_memcpy_h2d(cp._row_address(t, "value_cache", 0, p - 3), row.ctypes.data, row.nbytes))
            before = L.q4_prompt_passes()
            t.generate_ids_from(_LONG[:p + 20], p + 18, p)
            assert L.q4_prompt_passes() - before >= 2 and t.pos() == p + 18
            k, v = cp.read_rows(q4, t, p, 1)
            assert cp.finite(k[0]) and cp.finite(v[0]) and not cp.finite(k[1]) and not cp.finite(v[1]), p
    finally:
        q4.set_pass_context(256)
        t.close()


# ---- 8. hostile weights -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("trait", ["massive", "quant_edges"])
def test_hostile_weights(q4, models, trait):
    """massive residual channels, and pinned zero points / q == z groups / scales over two decades: a restated sum that parts from the original shows on
    such values where Gaussian weights hide it. 17 prompt tokens by passes, and q4_verify_tokens at position 30 at every first-wrong index."""
    path = models(NAME, trait)
    off = _off(q4, models, 2 * T + 1, trait=trait)
    assert cp.finite(off["k"]) and cp.finite(off["v"]) and cp.finite(off["logits"]), trait
    on = _run(q4, path, _LONG[:2 * T + 1])
    assert on["passes"] == 2
    _assert_same(off, on, "%s, 17 prompt tokens" % trait)
    want = _stepwise(q4, path, 30)
    assert all(cp.finite(x) for x in want["logits"])
    _verify_all_indices(q4, path, 30, want)


# ---- 9. not admitted, the switch on -------------------------------------------------------------------------------------------------------------------------------
NOT_ADMITTED = {
    "fp8": (NAME, dict(kv="fp8")),
    "fusion 1": (NAME, dict(level=1)),
    "fusion 0": (NAME, dict(level=0)),
    "head128_gqa": ("head128_gqa", {}),
    "tinyllama": ("tinyllama", {}),
}


@pytest.mark.parametrize("case", sorted(NOT_ADMITTED))
def test_not_admitted(q4, models, case):
    name, kw = NOT_ADMITTED[case]
    prompt = _LONG[:40]
    spec = dict(draft=4, ngram=3, min=1)
    on = _run(q4, models(name), prompt, steps=100, bound=S, spec=spec, drafter=lambda ring, room: [5] * room, **kw)
    off = _run(q4, models(name), prompt, steps=100, gqa=False, ingest=0, **kw)
    assert on["passes"] == 0 and on["stats"] == (0, 0, 0) and on["covers"] == [0] * 6, (case, on["passes"], on["stats"], on["covers"])
    _assert_same(off, on, case)


def test_multi_head_model_is_unchanged(q4, models):
    """ffn_pair7b with the switch on: the pass counts and the bytes it has with the switch off"""
    prompt = _LONG[:140]
    a = _run(q4, models(MHA), prompt, gqa=False)
    b = _run(q4, models(MHA), prompt, gqa=True)
    c = _run(q4, models(MHA), prompt, gqa=False, ingest=0)
    assert a["passes"] == b["passes"] == _expected_passes(140) and a["covers"] == b["covers"]
    _assert_same(a, b, "ffn_pair7b, switch on against off")
    _assert_same(c, b, "ffn_pair7b against the steps")


def test_down_form_knobs_keep_the_steps():
    """q4_set_ksplit / q4_set_half_tail exist in the profiling build only: tests/pass_gqa_prof_cases.py runs against it in a process of its own"""
    env = dict(os.environ, Q4_PROFILING_BUILD="1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "pass_gqa_prof_cases.py"), "-x", "-q", "-m", "gpu",
                        "-p", "no:cacheprovider"], env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert " passed" in r.stdout


# ---- 10. two models -------------------------------------------------------------------------------------------------------------------------------------------------
def test_two_models_alternate(q4, models):
    """an ffn_pair7b and a gqa7b_pair Transformer alternate generations with passes: each keeps its own scratch rows (hb rows of 11008 / 14336)"""
    L = q4.lib()
    pa, pb = _LONG[:41], _prompt(57, seed=21)
    fresh = {(name, len(p)): _run(q4, models(name), p) for name in (MHA, NAME) for p in (pa, pb)}
    ta, tb = q4.Transformer(models(MHA)), q4.Transformer(models(NAME), pass_gqa=True)
    try:
        for p in (pa, pb, pa):
            for name, t in ((MHA, ta), (NAME, tb)):
                before = L.q4_prompt_passes()
                toks = t.generate_ids(p, len(p) + GEN)[0].copy()
                want = fresh[name, len(p)]
                assert L.q4_prompt_passes() - before == want["passes"] == _expected_passes(len(p))
                k, v = cp.read_rows(q4, t, 0, t.pos())
                got = dict(tokens=toks, pos=t.pos(), k=k, v=v, logits=t.logits().view(np.uint16).copy(), rng=want["rng"])
                _assert_same(want, got, "%s, %d prompt tokens, alternating" % (name, len(p)))
                q4.check(L.q4_handoff_status(t.state))
    finally:
        ta.close()
        tb.close()


def test_built_after_a_freed_model(q4, models):
    a = _run(q4, models(MHA), _LONG[:41])
    b = _run(q4, models(NAME), _LONG[:41])
    assert a["passes"] == b["passes"] == 5
    _assert_same(_off(q4, models, 41), b, "gqa7b_pair behind a freed ffn_pair7b")


# ---- 11. the Llama-3 vocabulary -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 8])
def test_classifier_rows_at_vocabulary_128256(q4, n):
    """q4_verify_classifier at dim 4096, vocabulary 128256, row by row against q4_rmsnorm + q4_matmul_f16 (tests/test_speculative_gpu.py's pairing),
    the gigabyte of weights laid out on the device from one 501-row tile. Passes without the feature too: it pins the classifier pairing the feature
    makes usable for Llama-3."""
    L = q4.lib()
    vocab, dim = 128256, 4096
    r = np.random.default_rng(3)
    tile = (r.standard_normal((501, dim), dtype=np.float32) * 0.02).astype(np.float16)
    dw = q4.DevBuf(nbytes=vocab * dim * 2)
    rows = 0
    while rows < vocab:                              # the table: the tile again and again -- 256 copies of 4 MB, no gigabyte drawn on the host
        m = min(501, vocab - rows)
        q4.check(L.q4_memcpy_h2d(dw.ptr + rows * dim * 2, tile.ctypes.data, m * dim * 2))
        rows += m
    rms = q4.DevBuf((1.0 + 0.1 * r.uniform(-1, 1, dim)).astype(np.float16))
    x = r.standard_normal((8, dim), dtype=np.float32)
    x[1] = 0.0
    x[4] *= 30.0
    dx = q4.DevBuf(x.astype(np.float16))
    xn, lo, out = q4.DevBuf(nbytes=dim * 2), q4.DevBuf(nbytes=vocab * 2), q4.DevBuf(nbytes=8 * vocab * 2)
    q4.verify_classifier(out, dx, rms, dw, dim, vocab, n)
    got = out.get(np.uint16, 8 * vocab).reshape(8, vocab)
    for i in range(n):
        q4.check(L.q4_rmsnorm(xn.ptr, dx.ptr + i * dim * 2, rms.ptr, dim))
        q4.check(L.q4_matmul_f16(lo.ptr, xn.ptr, dw.ptr, dim, vocab, 1, 0, 0, 0, -1, 1.0))
        want = lo.get(np.uint16, vocab)
        bad = np.flatnonzero(got[i] != want)
        assert bad.size == 0, "row %d of %d: %d logits differ, first at %d" % (i, n, bad.size, bad[0])
    assert got[0].any() and not got[1].any()
