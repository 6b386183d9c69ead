"""Prompt passes and verify passes above position 255 (q4_set_pass_context; csrc/prompt_pass.hip's split-context attention launch and its merge;
DESIGN.md 3.7 / 3.8). A pass computes what the per-token steps compute, bit for bit, so "equal" below always means BYTE-equal against a run without
passes on a fresh Transformer: the token ring, every K / V row of both layers over the compared prefix (one snapshot export), the final logits. Expected
pass counts and speculation counters come from tests/pass_context_ref.py. Model: pass_long, Llama-2-7B's layer twice with a context of 2304."""
import ctypes as C

import numpy as np
import pytest

import pass_context_ref as ref
from llama_cu_awq_amd import synth

pytestmark = pytest.mark.gpu

SEED = 11
T = 8
GEN = 6               # generated steps behind a prompt
S = 2304              # pass_long's context, and the bound the tests raise the setting to
DIM = 4096
N_SPEC = 16           # the speculative runs' prompt
SPEC_STEPS = 1100


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    p = str(tmp_path_factory.mktemp("pass_context") / "pass_long.bin")
    synth.write_model(p, "pass_long", seed=SEED)
    return p


def _prompt(n, seed=5):
    r = np.random.default_rng(seed)
    return [1] + [int(x) for x in r.integers(3, 512, size=n - 1)]       # no EOS (2) inside


def _rows(t, n_pos):
    """every K / V row of every layer over positions [0, n_pos), with the tokens they belong to: one snapshot export"""
    snap = t.snapshot(n_pos)
    try:
        return np.frombuffer(snap.to_bytes(), dtype=np.uint8).copy()
    finally:
        snap.close()


def _x(q4, t, normalise=False):
    """RunState::x. A step of this model (vocabulary 512: q4_rmsnorm + q4_matmul_f16, no strips classifier) leaves it normalised in place, a verify pass
    leaves the accepted row's residual stream as it is (csrc/q4_passes.hip, verify_covers' comment); normalise: through the step's own q4_rmsnorm."""
    L = q4.lib()
    if normalise:
        q4.check(L.q4_rmsnorm(t.state.contents.x, t.state.contents.x, t.weights.contents.rms_final_weight, DIM))
    out = np.empty(DIM, dtype=np.uint16)
    q4.check(L.q4_stream_synchronize())
    q4.check(L.q4_memcpy_d2h(out.ctypes.data, t.state.contents.x, out.nbytes))
    return out


def _generate(q4, path, prompt, bound=S, ingest=T, graphs=1, start=0, warm=None, steps=None, second=None):
    """One generation on a fresh Transformer: dict(tokens, rows, logits, passes). warm: a prompt generated first on the same Transformer (start > 0
    reuses its prefix); second: (prompt, steps) generated afterwards -- the result is then the second generation's."""
    L = q4.lib()
    L.q4_set_use_graphs(graphs)
    L.q4_set_prompt_ingest(ingest)
    q4.set_pass_context(bound)
    t = q4.Transformer(path)
    try:
        if warm is not None:
            t.generate_ids(warm, len(warm) + GEN)
        steps = len(prompt) + GEN if steps is None else steps
        before = L.q4_prompt_passes()
        toks = t.generate_ids_from(prompt, steps, start)[0].copy()
        out = {"passes": L.q4_prompt_passes() - before}
        if second is not None:
            prompt, steps = second
            toks = t.generate_ids(prompt, steps)[0].copy()
        q4.check(L.q4_handoff_status(t.state))
        out.update(tokens=toks, rows=_rows(t, min(len(prompt), steps)), logits=t.logits().view(np.uint16).copy())
    finally:
        t.close()
        L.q4_set_prompt_ingest(T)
        L.q4_set_use_graphs(1)
        q4.set_pass_context(256)
    return out


def _assert_same(a, b, what):
    assert np.array_equal(a["tokens"], b["tokens"]), "%s: token rings differ" % what
    assert a["rows"].shape == b["rows"].shape, "%s: the exports differ in size" % what
    bad = np.flatnonzero(a["rows"] != b["rows"])
    assert bad.size == 0, "%s: K / V exports differ in %d bytes, first at byte %d of %d" % (what, bad.size, bad[0] if bad.size else -1, a["rows"].size)
    assert np.array_equal(a["logits"], b["logits"]), "%s: final logits differ in %d entries" % (what, int((a["logits"] != b["logits"]).sum()))


_OFF = {}


def _off(q4, model, n_prompt, graphs=1):
    """the per-token run (prompt ingest off), computed once per case and shared"""
    key = (n_prompt, graphs)
    if key not in _OFF:
        _OFF[key] = _generate(q4, model, _prompt(n_prompt), ingest=0, graphs=graphs)
        assert _OFF[key]["passes"] == 0
    return _OFF[key]


def _expected(n_prompt, bound=S, start=0, mode=1):
    return len(ref.prompt_passes(n_prompt, n_prompt + GEN, bound, S, start=start, mode=mode))


# ---- 1 - 5: prompt passes ---------------------------------------------------------------------------------------------------------------------------
def test_long_prompt_graphs(q4, model):
    """2200 prompt tokens and six generated steps: passes in chunks of 64, 128 and 256 positions and in the sixteen-chunk bin behind 2048"""
    off = _off(q4, model, 2200)
    on = _generate(q4, model, _prompt(2200))
    print("prompt passes: %d (expected %d)" % (on["passes"], _expected(2200)))
    _assert_same(off, on, "2200 prompt tokens, graphs")
    assert on["passes"] == _expected(2200) == 275


def test_default_bound_keeps_256(q4, model):
    """the same model with the setting left alone: passes below 256 only"""
    off = _off(q4, model, 600)
    on = _generate(q4, model, _prompt(600), bound=256)
    _assert_same(off, on, "600 prompt tokens, default bound")
    assert on["passes"] == 32


@pytest.mark.parametrize("graphs", [2, 0])
def test_eager(q4, model, graphs):
    """Eager bins run the bins' forms; without graphs a step is handed its own size as the bin, so positions 256 .. 510 run the one-block form (no
    pass), 511 the split form alone in its bin, and from 512 the split form with as many chunks as the position needs"""
    off = _off(q4, model, 600, graphs)
    on = _generate(q4, model, _prompt(600), graphs=graphs)
    print("graphs %d: prompt passes %d (expected %d)" % (graphs, on["passes"], _expected(600, mode=graphs)))
    _assert_same(off, on, "600 prompt tokens, graphs %d" % graphs)
    assert on["passes"] == _expected(600, mode=graphs) == (75 if graphs else 43)


@pytest.mark.parametrize("last", [510, 511, 512, 1022, 1023, 1024])
def test_bin_boundaries(q4, model, last):
    """prompts whose last prompt-only position is `last`: the pass in front of a bin end is cut there, a lone position is stepped"""
    n = last + 2
    off = _off(q4, model, n)
    on = _generate(q4, model, _prompt(n))
    _assert_same(off, on, "last prompt-only position %d" % last)
    assert on["passes"] == _expected(n) == (64 if last < 600 else 128)


def test_no_pass_spans_a_bin_end(q4, model):
    """resumed at 3, last prompt-only position 513: 65 passes -- a loop that let passes reach across 256 or 512 would run 64"""
    prompt = _prompt(515)
    off = _off(q4, model, 515)
    on = _generate(q4, model, prompt, start=3, warm=prompt[:3] + _prompt(12, seed=9)[1:])
    _assert_same(off, on, "resumed at 3")
    assert on["passes"] == _expected(515, start=3) == 65


def test_intermediate_bound(q4, model):
    off = _off(q4, model, 900)
    on = _generate(q4, model, _prompt(900), bound=700)
    _assert_same(off, on, "bound 700")
    assert on["passes"] == _expected(900, bound=700) == 88


def test_resume_at_300(q4, model):
    """generate_ids_from over a warm prefix of 300 positions (themselves ingested by passes): the full per-token run's bytes"""
    prompt = _prompt(700)
    off = _off(q4, model, 700)
    on = _generate(q4, model, prompt, start=300, warm=prompt[:300] + _prompt(40, seed=9)[1:])
    _assert_same(off, on, "resumed at 300")
    assert on["passes"] == _expected(700, start=300)


def test_clean_state_afterwards(q4, model):
    """a short generation behind a long one on the same Transformer equals a fresh one"""
    short = _prompt(T + 3, seed=21)
    fresh = _generate(q4, model, short)
    again = _generate(q4, model, _prompt(1100), second=(short, len(short) + GEN))
    off = _generate(q4, model, short, ingest=0)
    assert again["passes"] == _expected(1100)
    _assert_same(fresh, again, "second generation")
    _assert_same(off, again, "second generation against the steps")


# ---- 6 - 8: verify passes -----------------------------------------------------------------------------------------------------------------------------
def test_verify_admission(q4, model):
    t = q4.Transformer(model)
    try:
        assert t.verify_covers(248, 7) and not t.verify_covers(249, 7) and not t.verify_covers(300, 1)       # the default bound
        q4.set_pass_context(S)
        assert t.verify_covers(1016, 7) and not t.verify_covers(1017, 7) and t.verify_covers(1017, 6)
        assert t.verify_covers(2296, 7) and not t.verify_covers(2297, 7)                                     # seq_len
        assert t.verify_covers(248, 7) and not t.verify_covers(249, 7) and t.verify_covers(256, 7)           # the end of the V-slice bins is an end too
        q4.set_pass_context(700)
        assert t.verify_covers(692, 7) and not t.verify_covers(693, 7)
        q4.set_pass_context(256)
        assert not t.verify_covers(249, 7) and not t.verify_covers(300, 1)
    finally:
        q4.set_pass_context(256)
        t.close()


def _wrong(tok):
    w = (int(tok) + 1) % 512
    return w + 1 if w == 2 else w


def _oracle(R):
    return lambda ring, room: R[len(ring):len(ring) + room]


def _alternating(R):
    """by call: everything right, first wrong, second wrong, no draft (tests/test_speculative_gpu.py's)"""
    state = {"n": 0}

    def fn(ring, room):
        state["n"] += 1
        kind = state["n"] % 4
        d = [int(x) for x in R[len(ring):len(ring) + room]]
        if kind == 1:
            return d
        if kind == 2:
            return [_wrong(d[0])] + d[1:]
        if kind == 3:
            return d[:1] + [_wrong(d[1])] + d[2:] if len(d) > 1 else d
        return []
    return fn


def _spec_run(q4, path, steps, bound=S, spec=None, drafter=None, groups=False):
    L = q4.lib()
    prompt = _prompt(N_SPEC)
    q4.set_pass_context(bound)
    t = q4.Transformer(path)
    try:
        if spec is not None:
            t.set_speculative(**spec)
        if drafter is not None:
            t.set_drafter(drafter)
        out = {"tokens": t.generate_ids(prompt, steps)[0].copy()}
        q4.check(L.q4_handoff_status(t.state))
        out.update(rows=_rows(t, min(steps, len(out["tokens"]) - 1)), logits=t.logits().view(np.uint16).copy(), x=_x(q4, t), stats=t.spec_stats(), pos=t.pos())
        if groups:       # what the loop queues at a generating position without a draft (q4_steps_that_fit, asked of the live model)
            L.q4_steps_that_fit.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
            cfg = C.cast(L.q4_transformer_config(t.h), C.c_void_p)
            out["groups"] = {pos: L.q4_steps_that_fit(pos, len(prompt), steps, cfg, t.sampler) for pos in range(len(prompt) - 1, steps)}
    finally:
        t.close()
        q4.set_pass_context(256)
    return out


_SPEC_OFF = {}


def _spec_off(q4, model, steps=SPEC_STEPS):
    if steps not in _SPEC_OFF:
        _SPEC_OFF[steps] = _spec_run(q4, model, steps, groups=steps == SPEC_STEPS)
        assert _SPEC_OFF[steps]["stats"] == (0, 0, 0) and len(_SPEC_OFF[steps]["tokens"]) == steps + 1
    return _SPEC_OFF[steps]


_SHORTENED = []


@pytest.mark.parametrize("kind", ["oracle", "alternating"])
def test_speculative_loop(q4, model, kind):
    """a 16-token prompt to 1100 steps, seven drafts per pass: the run without speculation, byte for byte, and the counters of the replay"""
    off = _spec_off(q4, model)
    R = off["tokens"]
    make = _oracle if kind == "oracle" else _alternating
    on = _spec_run(q4, model, SPEC_STEPS, spec=dict(draft=7, ngram=3, min=1), drafter=make(R))
    _assert_same(off, on, "%s drafter" % kind)
    want, passes = ref.replay(R, N_SPEC, SPEC_STEPS, make(R), 7, lambda pos: off["groups"][pos], S, S)
    print("%s: passes, drafted, accepted = %s (expected %s)" % (kind, on["stats"], want))
    assert on["stats"] == want
    assert any(512 <= pos and pos + d < 1024 for pos, d, _ in passes) and any(pos >= 1024 for pos, d, _ in passes)
    assert all(ref.bin_end(pos) > pos + d for pos, d, _ in passes)
    _SHORTENED.extend(p for p in passes if p[1] < 7 and p[0] + p[1] + 1 == ref.bin_end(p[0]))
    if kind == "oracle":
        assert want[1] == want[2]
    else:
        assert _SHORTENED, "no draft was shortened at a bin end in either run"
    # with the default bound the same drafter stops at 256
    if kind == "oracle":
        low = _spec_run(q4, model, SPEC_STEPS, bound=256, spec=dict(draft=7, ngram=3, min=1), drafter=make(R))
        _assert_same(off, low, "oracle drafter, default bound")
        assert low["stats"] == ref.replay(R, N_SPEC, SPEC_STEPS, make(R), 7, lambda pos: off["groups"][pos], 256, S)[0]
        assert low["stats"][0] < want[0]


@pytest.mark.parametrize("first_wrong", [7, 3])
def test_primitive_above_1024(q4, model, first_wrong):
    """q4_verify_tokens at position 1030 with seven drafts -- the run's own continuation, or wrong at index 3 -- against stepping to where the pass
    ends: the position, the ring, RunState::logits, RunState::x and the rows"""
    R = _spec_off(q4, model)["tokens"]
    p, D, k = 1030, 7, first_wrong
    want = _spec_off(q4, model, p + k + 1)
    assert np.array_equal(want["tokens"], R[:p + k + 2])
    q4.set_pass_context(S)
    t = q4.Transformer(model)
    try:
        t.generate_ids(R[:N_SPEC], p)
        assert t.pos() == p and t.verify_covers(p, D)
        drafts = [int(x) for x in R[p + 1:p + 1 + D]]
        if k < D:
            drafts[k] = _wrong(drafts[k])
        emitted, acc = t.verify(drafts)
        assert acc == k and emitted.tolist() == R[p + 1:p + k + 2].tolist()
        assert t.pos() == p + k + 1 == want["pos"]
        assert [t.token(i) for i in range(p + k + 2)] == R[:p + k + 2].tolist()
        assert t.spec_stats() == (1, D, k)
        assert np.array_equal(t.logits().view(np.uint16), want["logits"]), "logits behind the pass"
        rows = _rows(t, p + k + 1)
        assert rows.shape == want["rows"].shape and np.array_equal(rows, want["rows"]), "K / V rows behind the pass"
        assert np.array_equal(_x(q4, t, normalise=True), want["x"]), "x behind the pass"
        q4.check(q4.lib().q4_handoff_status(t.state))
    finally:
        q4.set_pass_context(256)
        t.close()


# ---- the CLI's setting ---------------------------------------------------------------------------------------------------------------------------------
def test_cli_setting(tmp_path):
    """Q4_PASS_CONTEXT=<integer> beside Q4_SPECULATIVE: a malformed value ends the run with a message that names it; a good one changes no output"""
    import os
    import re
    import subprocess
    from conftest import GOLDEN, ROOT
    exe = os.path.join(ROOT, "llama_cu_awq_amd", "bin", "llama2_q4")
    path = str(tmp_path / "cli.bin")
    synth.write_model(path, (256, 352, 2, 4, 4, 32000, 256, 10000.0), seed=31)

    def run(value):
        env = dict(os.environ)
        env.pop("Q4_PASS_CONTEXT", None)
        if value is not None:
            env["Q4_PASS_CONTEXT"] = value
        r = subprocess.run([exe, path, "-n", "24", "-i", "Hello", "-t", "0", "-z", os.path.join(GOLDEN, "tokenizer.bin")], env=env, capture_output=True,
                           text=True, timeout=120, errors="replace")
        return r.returncode, re.sub(r"achieved tok/s.*", "", r.stdout), r.stderr
    rc0, out0, err0 = run(None)
    assert rc0 == 0, err0
    for bad in ("abc", "12x", "-4", " 300", "1e3", "99999999999"):
        rc, _, err = run(bad)
        assert rc != 0 and "Q4_PASS_CONTEXT" in err and bad in err, (bad, rc, err)
    for good in ("2048", "0", "256"):
        rc, out, err = run(good)
        assert rc == 0 and out == out0, (good, err)
