"""No launch's result depends on a K / V cache row at or above the position it computes. Rejected drafts, context shift, a restored
snapshot and prefix reuse all leave rows above the position; csrc/prompt_pass.hip promises that a masked lane multiplies its zero probability by the V
row the step's clamp would have handed it, never by the row it holds, and the step's attention bounds its buffer descriptors at `size` rows. Here
those rows hold poison (tests/cache_poison.py: NaN everywhere, or +-65504 with +inf at every 7th half), written after the build and after any warm
generation, and every case must give, BYTE for byte, what its clean twin on a fresh Transformer gives: the ring, the rows below the final position, the
final logits. A kernel that reads one row too far and multiplies it by a zero probability turns NaN here. The poison is data in rows the kernels are
specified not to read; loading it faults nowhere.

Behind every model case the rows from eight above the final position (a pass may write PROMPT_PASS_MAX = 8 rows ahead of where the run ends) to the
end of the cache must still hold the pattern: nothing writes further.

  control   a NaN V row BELOW the position makes the next step's logits non-finite: the poison reaches the attention kernels through that pointer and
            layout (the helper's offsets are checked against q4_get_kv_row beside it)
  1. steps  head128 (context 1100), 600 steps, graphs and none, the default fusion level and level 1: the fused attention -> o-proj role below 512
            (V-slice forms), the split-context forms whose graph bin is larger than the position (bins 1024 and 2048 -> seq_len), and without graphs the
            one-block form handed its own size (257 .. 511) and the split form with as many chunks as the position needs
  2. steps  head64_long (grouped-query, head 64, context 1300), 600 steps, graphs
  3. prompt passes  ffn_pair7b, 140 prompt tokens and six steps, graphs and eager bins, from 0 and resumed at 5 over a warm prefix (the rows the warm run
            left above 5 are what the poison overwrites): prompt_gemv_kernel, prompt_attention_kernel
  4. split passes  pass_long, bound 2304, 1040 prompt tokens and six steps, passes of eight and of five: prompt_split_attention_kernel<2 | 4 | 8>,
            prompt_merge_kernel, chunks wholly above a token's position
  5. verify passes  ffn_pair7b with the alternating drafter to 150 steps (rejected drafts write rows above the position in the middle of the poison);
            pass_long, the primitive at position 520 with seven drafts, wrong at index 3
  6. q4_multi_head_attention with the rows above `pos` poisoned in the host arrays: the one-block form and the split form, against zeros there

The FP8 cache is not covered: its rows and exponent arrays need a poison format of their own."""
import numpy as np
import pytest

import cache_poison as cp
import pass_context_ref as ref
from llama_cu_awq_amd import synth

pytestmark = pytest.mark.gpu

SEED = 11
T = 8
GEN = 6
S = 2304
AHEAD = 8                 # PROMPT_PASS_MAX: how far above the final position a pass may have written


@pytest.fixture(scope="module")
def models(tmp_path_factory):
    d = tmp_path_factory.mktemp("stale_rows")
    made = {}

    def get(name):
        if name not in made:
            made[name] = str(d / (name + ".bin"))
            synth.write_model(made[name], name, seed=SEED)
        return made[name]
    return get


def _prompt(n, seed=5):
    r = np.random.default_rng(seed)
    return [1] + [int(x) for x in r.integers(3, 512, size=n - 1)]       # no EOS (2) inside


def _wrong(tok):
    w = (int(tok) + 1) % 512
    return w + 1 if w == 2 else w


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


def _run(q4, path, prompt, steps, pattern=None, ingest=0, graphs=1, bound=256, level=None, start=0, warm=None, drafter=None, verify=None):
    """One generation on a fresh Transformer, its cache poisoned from row `start` first when a pattern is given: dict(tokens, k, v (the rows below the
    final position), logits, pos, passes, stats). warm: a prompt generated first (start > 0 reuses its prefix; the poison follows it). drafter: the
    loop speculates with seven drafts. verify: drafts for one q4_verify_tokens behind the generation. With a pattern, the rows from AHEAD above the
    final position must still hold it."""
    L = q4.lib()
    default = L.q4_get_prompt_ingest()
    try:
        if level is not None:
            L.q4_set_fusion(level)
        L.q4_set_use_graphs(graphs)
        L.q4_set_prompt_ingest(ingest)
        q4.set_pass_context(bound)
        t = q4.Transformer(path)
        try:
            if warm is not None:
                t.generate_ids(warm, len(warm) + GEN)
            if pattern is not None:
                cp.poison(q4, t, start, pattern)
            if drafter is not None:
                t.set_speculative(draft=7, ngram=3, min=1)
                t.set_drafter(drafter)
            before = L.q4_prompt_passes()
            toks = t.generate_ids_from(prompt, steps, start)[0].copy()
            out = {"passes": L.q4_prompt_passes() - before}
            if verify is not None:
                assert t.pos() == steps and t.verify_covers(steps, len(verify))
                emitted, acc = t.verify(verify)
                toks = np.array([t.token(i) for i in range(t.pos() + 1)], dtype=np.int32)
                out["accepted"] = acc
            q4.check(L.q4_handoff_status(t.state))
            pos = t.pos()
            out.update(tokens=toks, pos=pos, logits=t.logits().view(np.uint16).copy(), stats=t.spec_stats())
            out["k"], out["v"] = cp.read_rows(q4, t, 0, pos)
            if pattern is not None and pos + AHEAD < t.config.seq_len:
                cp.assert_untouched(q4, t, pos + AHEAD, pattern, "final position %d" % pos)
        finally:
            t.close()
    finally:
        if level is not None:
            L.q4_set_fusion(q4.DEFAULT_FUSION)
        L.q4_set_prompt_ingest(default)
        L.q4_set_use_graphs(1)
        q4.set_pass_context(256)
    return out


def _assert_twin(clean, got, what):
    assert cp.finite(clean["logits"]) and cp.finite(clean["k"]) and cp.finite(clean["v"]), "%s: the clean run is not finite" % what
    assert got["pos"] == clean["pos"] and np.array_equal(got["tokens"], clean["tokens"]), "%s: token rings differ" % what
    for name in ("k", "v"):
        bad = np.argwhere((got[name] != clean[name]).any(axis=2))
        assert bad.size == 0, "%s: %s rows differ from the clean run's, first (layer, position) %s" % (
            what, name.upper(), [tuple(int(i) for i in x) for x in bad[:8]])
    assert np.array_equal(got["logits"], clean["logits"]), "%s: final logits differ in %d entries (finite: %s)" % (
        what, int((got["logits"] != clean["logits"]).sum()), cp.finite(got["logits"]))
    assert got["passes"] == clean["passes"] and got["stats"] == clean["stats"]


_CLEAN = {}


def _clean(q4, key, path, prompt, steps, **kw):
    """the clean twin, once per case and shared by the patterns"""
    if key not in _CLEAN:
        _CLEAN[key] = _run(q4, path, prompt, steps, **kw)
    return _CLEAN[key]


# ---- the helper and the control ---------------------------------------------------------------------------------------------------------------------
def test_helper_offsets(q4, models):
    """after poison(t, 5, ...): q4_get_kv_row's row 4 is what it was, rows 5 and seq_len - 1 are the pattern, in the first and the last layer; and
    read_rows returns what q4_get_kv_row returns"""
    t = q4.Transformer(models("ffn_pair7b"))
    try:
        t.generate_ids(_prompt(10), 8)                      # rows 0 .. 7 hold the run's values
        last_layer, last_row = t.config.n_layers - 1, t.config.seq_len - 1
        before = {layer: t.kv_row(layer, 4) for layer in (0, last_layer)}
        assert all(k.any() and v.any() for k, v in before.values())
        for pattern in cp.PATTERNS:
            cp.poison(q4, t, 5, pattern)
            want = cp.pattern_row(pattern, 4096)
            rk, rv = cp.read_rows(q4, t, 4, 2)
            for layer in (0, last_layer):
                k4, v4 = t.kv_row(layer, 4)
                assert np.array_equal(k4.view(np.uint16), before[layer][0].view(np.uint16)) and np.array_equal(v4.view(np.uint16), before[layer][1].view(np.uint16))
                assert np.array_equal(rk[layer, 0], k4.view(np.uint16)) and np.array_equal(rv[layer, 0], v4.view(np.uint16))
                for row in (5, last_row):
                    k, v = t.kv_row(layer, row)
                    assert np.array_equal(k.view(np.uint16), want) and np.array_equal(v.view(np.uint16), want), (pattern, layer, row)
                assert np.array_equal(rk[layer, 1], want) and np.array_equal(rv[layer, 1], want)
            cp.assert_untouched(q4, t, 5, pattern)
        huge = cp.pattern_row("huge", 4096).view(np.float16)
        assert huge[0] == 65504 and huge[1] == -65504 and np.isposinf(huge[6]) and np.isposinf(huge[13]) and np.isfinite(huge[:6]).all()
        assert np.isnan(cp.pattern_row("nan", 4096).view(np.float16)).all()
    finally:
        t.close()


def test_control_a_poisoned_row_below_the_position_shows(q4, models):
    """20 positions, then NaN in the V rows from row 3 -- BELOW the position --, then one more step: its logits are not finite. The tests below can
    fail: the poison sits where the attention kernels read."""
    t = q4.Transformer(models("ffn_pair7b"))
    try:
        t.generate_ids(_prompt(17), 20)
        assert t.pos() == 20 and np.isfinite(t.logits().astype(np.float32)).all()
        cp.poison(q4, t, 3, "nan", caches=("value_cache",))
        t.run_transformer_at(20, True)
        q4.synchronize()
        assert not np.isfinite(t.logits().astype(np.float32)).all()
    finally:
        t.close()


# ---- 1, 2: steps only -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", cp.PATTERNS)
@pytest.mark.parametrize("level", ["default", 1])
@pytest.mark.parametrize("graphs", [1, 0])
def test_steps_head128(q4, models, graphs, level, pattern):
    level = q4.DEFAULT_FUSION if level == "default" else level
    kw = dict(graphs=graphs, level=level)
    clean = _clean(q4, ("head128", graphs, level), models("head128"), [1, 5, 9], 600, **kw)
    got = _run(q4, models("head128"), [1, 5, 9], 600, pattern=pattern, **kw)
    assert clean["pos"] == 600 and clean["passes"] == 0
    _assert_twin(clean, got, "head128, graphs %d, level %d, %s" % (graphs, level, pattern))


@pytest.mark.parametrize("pattern", cp.PATTERNS)
def test_steps_head64_grouped_query(q4, models, pattern):
    clean = _clean(q4, "head64_long", models("head64_long"), [1, 5, 9], 600)
    got = _run(q4, models("head64_long"), [1, 5, 9], 600, pattern=pattern)
    assert clean["pos"] == 600
    _assert_twin(clean, got, "head64_long, %s" % pattern)


# ---- 3, 4: prompt passes ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", cp.PATTERNS)
@pytest.mark.parametrize("start", [0, 5])
@pytest.mark.parametrize("graphs", [1, 2])
def test_prompt_passes(q4, models, graphs, start, pattern):
    prompt = _prompt(140)
    kw = dict(ingest=T, graphs=graphs, start=start, warm=prompt[:5] + _prompt(12, seed=9)[1:] if start else None)
    clean = _clean(q4, ("ffn_pair7b", graphs, start), models("ffn_pair7b"), prompt, len(prompt) + GEN, **kw)
    got = _run(q4, models("ffn_pair7b"), prompt, len(prompt) + GEN, pattern=pattern, **kw)
    assert clean["passes"] == len(ref.prompt_passes(140, 146, 256, 300, start=start)) and clean["pos"] == 146
    _assert_twin(clean, got, "ffn_pair7b, graphs %d, start %d, %s" % (graphs, start, pattern))


@pytest.mark.parametrize("pattern", cp.PATTERNS)
@pytest.mark.parametrize("ingest", [8, 5])
def test_split_passes(q4, models, ingest, pattern):
    prompt = _prompt(1040)
    kw = dict(ingest=ingest, bound=S)
    clean = _clean(q4, ("pass_long", ingest), models("pass_long"), prompt, len(prompt) + GEN, **kw)
    got = _run(q4, models("pass_long"), prompt, len(prompt) + GEN, pattern=pattern, **kw)
    assert clean["passes"] == len(ref.prompt_passes(1040, 1046, S, S, ingest=ingest)) and clean["pos"] == 1046
    _assert_twin(clean, got, "pass_long, passes of %d, %s" % (ingest, pattern))


# ---- 5: verify passes ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", cp.PATTERNS)
def test_speculative_loop(q4, models, pattern):
    """a 17-token prompt to 150 steps with the alternating drafter: the rejected drafts' rows land above the position, among the poison, and are the
    next pass's stale rows"""
    prompt = _prompt(17)
    R = _clean(q4, "spec_off", models("ffn_pair7b"), prompt, 150, ingest=T)["tokens"]
    assert len(R) == 151
    clean = _clean(q4, "spec_on", models("ffn_pair7b"), prompt, 150, ingest=T, drafter=_alternating(R))
    got = _run(q4, models("ffn_pair7b"), prompt, 150, pattern=pattern, ingest=T, drafter=_alternating(R))
    assert np.array_equal(clean["tokens"], R) and clean["stats"][0] >= 10 and 0 < clean["stats"][2] < clean["stats"][1]
    _assert_twin(clean, got, "ffn_pair7b, alternating drafter, %s" % pattern)


@pytest.mark.parametrize("pattern", cp.PATTERNS)
def test_verify_primitive_in_a_split_bin(q4, models, pattern):
    """q4_verify_tokens at position 520 of pass_long with seven drafts, wrong at index 3: rows 524 .. 527 are the rejected drafts'"""
    prompt, p, D, k = _prompt(16), 520, 7, 3
    R = _clean(q4, "long_off", models("pass_long"), prompt, p + D + 1, ingest=T, bound=S)["tokens"]
    drafts = [int(x) for x in R[p + 1:p + 1 + D]]
    drafts[k] = _wrong(drafts[k])
    clean = _clean(q4, "long_verify", models("pass_long"), prompt, p, ingest=T, bound=S, verify=drafts)
    got = _run(q4, models("pass_long"), prompt, p, pattern=pattern, ingest=T, bound=S, verify=drafts)
    assert clean["accepted"] == k == got["accepted"] and clean["pos"] == p + k + 1 and np.array_equal(clean["tokens"], R[:p + k + 2])
    _assert_twin(clean, got, "pass_long, verify at %d, %s" % (p, pattern))


# ---- 6: the public attention entry ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", cp.PATTERNS)
@pytest.mark.parametrize("heads,kv_mul,hs,pos,seq,scratch", [(8, 1, 128, 300, 512, False), (8, 1, 128, 600, 2048, True), (8, 4, 64, 600, 2048, True)])
def test_attention_entry(q4, heads, kv_mul, hs, pos, seq, scratch, pattern):
    """q4_multi_head_attention over caches of `seq` rows whose rows above `pos` hold the poison: the bytes of the same call over zeros there. Without
    scratch the one-block form, with it the split form (three chunks of 256 in a bin of 2048)."""
    r = np.random.default_rng(pos + hs + kv_mul)
    dim, kv_dim = heads * hs, heads // kv_mul * hs
    q = r.standard_normal(dim).astype(np.float16)
    K = np.zeros((seq, kv_dim), dtype=np.float16)
    V = np.zeros((seq, kv_dim), dtype=np.float16)
    K[:pos + 1] = (r.standard_normal((pos + 1, kv_dim)) * 0.5).astype(np.float16)
    V[:pos + 1] = r.standard_normal((pos + 1, kv_dim)).astype(np.float16)

    def run(K, V):
        dq, dk, dv, do = q4.DevBuf(q), q4.DevBuf(K), q4.DevBuf(V), q4.DevBuf(nbytes=dim * 2)
        dpos = q4.DevBuf(np.array([pos], dtype=np.int32))
        att = q4.DevBuf(nbytes=heads * max(seq, dim) * 2 * 2) if scratch else None
        q4.check(q4.lib().q4_multi_head_attention(do.ptr, dq.ptr, dk.ptr, dv.ptr, att.ptr if att else None, heads, hs, kv_mul, seq, dpos.ptr))
        q4.synchronize()
        return do.get(np.uint16, dim)
    clean = run(K, V)
    assert cp.finite(clean) and clean.any()
    Kp, Vp = K.copy(), V.copy()
    Kp.view(np.uint16)[pos + 1:] = cp.pattern_row(pattern, kv_dim)
    Vp.view(np.uint16)[pos + 1:] = cp.pattern_row(pattern, kv_dim)
    got = run(Kp, Vp)
    assert np.array_equal(got, clean), "%d of %d outputs differ (finite: %s)" % (int((got != clean).sum()), dim, cp.finite(got))
