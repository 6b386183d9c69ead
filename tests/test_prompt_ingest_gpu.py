"""Prompt passes (csrc/prompt_pass.h, q4_set_prompt_ingest): the token loop runs up to T = 8 consecutive prompt-only positions as one
pass over the weights. Same arithmetic in the same order as the per-token steps, so every K / V row, the final logits and the generated tokens must agree
BIT FOR BIT with the switch off -- and wherever a pass is not admitted the loop must run exactly as before (the counter q4_prompt_passes says which)."""
import numpy as np
import pytest

from llama_cu_awq_amd import synth

pytestmark = pytest.mark.gpu

T = 8
GEN = 6            # generated steps behind the prompt


@pytest.fixture(scope="module")
def models(tmp_path_factory):
    d = tmp_path_factory.mktemp("prompt_ingest")
    out = {}
    for name in ("ffn_pair7b", "ffn_pair_ragged", "tiny"):
        p = str(d / (name + ".bin"))
        synth.write_model(p, name, seed=11)
        out[name] = p
    return out


def _prompt(n, seed=5):
    r = np.random.default_rng(seed)
    return [1] + [int(x) for x in r.integers(3, 512, size=n - 1)]       # no EOS (2) inside


def _expected_passes(n_prompt, start=0):
    """positions start .. n_prompt - 2 are prompt-only; a pass takes up to T of them, at least 2, all below 256"""
    m = max(0, min(n_prompt - 1, 256) - start)
    return m // T + (1 if m % T >= 2 else 0)


def _state(t, n_prompt):
    kv = np.stack([np.concatenate([np.concatenate(t.kv_row(l, pos)) for l in range(t.config.n_layers)]) for pos in range(n_prompt)])
    return kv.view(np.uint16).copy(), t.logits().view(np.uint16).copy()


def _generate(q4, path, ingest, graphs, prompt, start=0, warm=None, **kw):
    """(tokens, K / V rows of every layer and prompt position, final logits, passes run) of one generation on a fresh Transformer; warm: a prompt
    generated first on the same Transformer (its prefix is what start > 0 reuses)"""
    L = q4.lib()
    default = L.q4_get_prompt_ingest()
    L.q4_set_use_graphs(graphs)
    L.q4_set_prompt_ingest(ingest)
    t = q4.Transformer(path, **kw)
    try:
        if warm is not None:
            t.generate_ids(warm, len(warm) + GEN)
        before = L.q4_prompt_passes()
        toks = t.generate_ids_from(prompt, len(prompt) + GEN, start)[0].copy()
        passes = L.q4_prompt_passes() - before
        q4.check(L.q4_handoff_status(t.state))
        kv, logits = _state(t, len(prompt))
    finally:
        t.close()
        L.q4_set_prompt_ingest(default)
        L.q4_set_use_graphs(1)
    return toks, kv, logits, passes


def _assert_same(a, b, what):
    assert np.array_equal(a[0], b[0]), "%s: token rings differ: %s vs %s" % (what, a[0], b[0])
    assert np.array_equal(a[1], b[1]), "%s: K / V rows differ at positions %s" % (what, np.unique(np.argwhere(a[1] != b[1])[:, 0])[:8])
    assert np.array_equal(a[2], b[2]), "%s: final logits differ in %d entries" % (what, int((a[2] != b[2]).sum()))


_OFF = {}


def _off(q4, models, name, graphs, n_prompt):
    """the per-token result, computed once per case and shared"""
    key = (name, graphs, n_prompt)
    if key not in _OFF:
        _OFF[key] = _generate(q4, models[name], 0, graphs, _prompt(n_prompt))
        assert _OFF[key][3] == 0
    return _OFF[key]


def test_default_is_on(q4):
    assert q4.lib().q4_get_prompt_ingest() == T


@pytest.mark.parametrize("graphs", [1, 2])
@pytest.mark.parametrize("n_prompt", [2, 3, T, T + 1, 2 * T + 1, 130, 140])
@pytest.mark.parametrize("name", ["ffn_pair7b", "ffn_pair_ragged"])
def test_bytes(q4, models, name, n_prompt, graphs):
    """Switch on against switch off, graphs and eager bins: every K / V row of every layer and prompt position, the final logits and the token ring are
    byte-equal, and the counter advanced by the expected number of passes. 130 and 140 cross the bin 128 -> 256 boundary inside a pass sequence."""
    off = _off(q4, models, name, graphs, n_prompt)
    on = _generate(q4, models[name], T, graphs, _prompt(n_prompt))
    assert on[3] == _expected_passes(n_prompt)
    _assert_same(off, on, "%s, %d prompt tokens, graphs %d" % (name, n_prompt, graphs))


def test_smaller_passes(q4, models):
    """q4_set_prompt_ingest(3): passes of three positions (and a last one of two)"""
    off = _off(q4, models, "ffn_pair7b", 1, 2 * T + 1)
    on = _generate(q4, models["ffn_pair7b"], 3, 1, _prompt(2 * T + 1))
    assert on[3] == 16 // 3 + 0       # 16 prompt-only positions: five passes of three, the last position per token
    _assert_same(off, on, "passes of three")


def test_positions_from_256_run_per_token(q4, models):
    """A 270-token prompt: passes below position 256 only, everything equal"""
    off = _off(q4, models, "ffn_pair7b", 1, 270)
    on = _generate(q4, models["ffn_pair7b"], T, 1, _prompt(270))
    assert on[3] == 256 // T
    _assert_same(off, on, "270 prompt tokens")


def test_logprobs_keep_the_steps(q4, models):
    """log-probability records describe the prompt steps' logits: no pass, the same results"""
    off = _off(q4, models, "ffn_pair7b", 1, 2 * T + 1)
    on = _generate(q4, models["ffn_pair7b"], T, 1, _prompt(2 * T + 1), logprobs=0)
    assert on[3] == 0
    _assert_same(off, on, "records on")


def test_reused_prefix(q4, models):
    """generate_ids_from over a reused prefix of five positions: the passes start at position 5 (one of them straddles position 128), and the result is the
    full per-token run's"""
    prompt = _prompt(140)
    warm = prompt[:5] + _prompt(12, seed=9)[1:]
    off = _off(q4, models, "ffn_pair7b", 1, 140)
    on = _generate(q4, models["ffn_pair7b"], T, 1, prompt, start=5, warm=warm)
    assert on[3] == _expected_passes(140, 5)
    _assert_same(off, on, "resumed at 5")


@pytest.mark.parametrize("level", [1, 0])
def test_fusion_levels_without_waits_keep_the_steps(q4, models, level):
    L = q4.lib()
    L.q4_set_fusion(level)
    try:
        on = _generate(q4, models["ffn_pair7b"], T, 1, _prompt(2 * T + 1))
    finally:
        L.q4_set_fusion(q4.DEFAULT_FUSION)
    assert on[3] == 0
    assert len(on[0]) >= 2 * T + 1


def test_other_geometry_keeps_the_steps(q4, models):
    on = _generate(q4, models["tiny"], T, 1, _prompt(2 * T + 1))
    off = _generate(q4, models["tiny"], 0, 1, _prompt(2 * T + 1))
    assert on[3] == 0 and off[3] == 0
    _assert_same(off, on, "tiny")


def test_same_state_afterwards(q4, models):
    """A second generation with another prompt on the same Transformer equals a fresh one: no stale position, tag or scratch vector remains"""
    second = _prompt(T + 3, seed=21)
    fresh = _generate(q4, models["ffn_pair7b"], T, 1, second)
    again = _generate(q4, models["ffn_pair7b"], T, 1, second, warm=_prompt(2 * T + 1))
    off = _generate(q4, models["ffn_pair7b"], 0, 1, second)
    assert fresh[3] == again[3] == _expected_passes(T + 3)
    _assert_same(fresh, again, "second generation")
    _assert_same(off, again, "second generation against the steps")
