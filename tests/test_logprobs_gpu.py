"""Per-token log-probability records (csrc/q4_logprobs.hip, q4_set_logprobs): the kernel on crafted logits against the float64 reference, the
records inside the decode step in every graph form, that nothing else changes, scoring, and the life cycle of the switch.

The bound everything is held to is logprobs_ref.bound: 2^-24 * (2 |l - m| + 3 ln n + 64)."""
import numpy as np
import pytest

import logprobs_ref
from llama_cu_awq_amd import synth

pytestmark = pytest.mark.gpu

ERR_ARG = 5
PROMPT = [1, 20, 300, 7, 45, 101, 13, 250, 77, 9, 410]          # 11 tokens: prompt steps, the prompt -> generate boundary, full eight-step groups
STEPS = 40
SAMPLED = (0.8, 0.9)


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. the kernel on crafted logits
HIGH = 65536          # a vocabulary beyond 16 bits of token id: every entry that decides a result sits at an id >= HIGH


def _distributions(rng, n, k, lo=0):
    """(name, fp16 logits, target) -- the target lies outside the top k wherever n allows it. lo > 0: the same distributions with the entries below id lo
    moved 40 down (-60000 becomes -60032; the one at +60000 is placed above lo), so the maximum, its ties, the top k + 6 and the target all have ids >= lo."""
    out = []
    for scale in (1.0, 8.0):
        out.append(("normal x%g" % scale, (rng.standard_normal(n) * scale).astype(np.float16)))
    out.append(("all equal", np.full(n, 1.5, dtype=np.float16)))
    x = rng.standard_normal(n).astype(np.float16)
    dup = np.sort(x[lo:])[::-1][min(k, n - lo - 1)]             # the value at rank k: the duplicates straddle it
    x[lo + rng.choice(n - lo, size=min(300, max(1, (n - lo) // 2)), replace=False)] = dup
    out.append(("duplicates at rank k", x))
    x = np.full(n, -60000.0, dtype=np.float16)
    x[int(rng.integers(lo, n))] = 60000.0
    out.append(("one at +60000", x))
    x = (rng.standard_normal(n) * 2.0).astype(np.float16)
    if n > 1:
        x[rng.choice(n, size=n // 2, replace=False)] = -np.inf
    out.append(("-inf on half", x))
    x = (rng.standard_normal(n) * 3.0).astype(np.float16)
    x[::3] = np.float16(-0.0)                                   # signed zeros tie with each other
    x[1::3] = np.float16(0.0)
    out.append(("signed zeros", x))
    res = []
    for name, x in out:
        if lo:
            x[:lo] = (x[:lo].astype(np.float32) - 40.0).astype(np.float16)
        order = np.lexsort((np.arange(n), -x.astype(np.float64)))
        res.append((name, x, int(order[min(n - 1, k + 5)])))
    return res


def _launch(q4, x, k, target):
    n = x.shape[0]
    dl = q4.DevBuf(x)
    dt = q4.DevBuf(np.array([target], dtype=np.int32))
    lse, tlp = q4.DevBuf(nbytes=4), q4.DevBuf(nbytes=4)
    ids, top = q4.DevBuf(nbytes=4 * max(k, 1)), q4.DevBuf(nbytes=4 * max(k, 1))
    q4.logprob_topk(dl, n, k, dt, lse, tlp, ids, top)
    q4.synchronize()
    return lse.get(np.float32, 1), tlp.get(np.float32, 1), ids.get(np.int32, max(k, 1))[:k], top.get(np.float32, max(k, 1))[:k]


@pytest.mark.parametrize("n", [1, 8, 20, 1000, 1027, 32000, 32768, 32776, 40000, 128256, 128259])
def test_kernel_matches_the_reference(q4, n):
    """(128256 / 128259: Llama-3's vocabulary and one that is no multiple of eight -- sixteen runs of the looping path per thread; q4_logprob_topk admits
    them up to k = 47, logprobs_size_ok. Every deciding id lies beyond 16 bits there, asserted on the reference's answer.)"""
    rng = np.random.default_rng(1000 + n)
    lo = HIGH if n > HIGH else 0
    highest = 0
    for k in (0, 1, 5, 20):
        if k > n:
            continue
        for name, x, target in _distributions(rng, n, k, lo):
            what = "n %d k %d %s" % (n, k, name)
            lse, tlp, ids, top = _launch(q4, x, k, target)
            rids, rlp = logprobs_ref.topk(x, k)
            want_lse, all_lp = logprobs_ref.lse(x), logprobs_ref.logprobs(x)
            with np.errstate(invalid="ignore"):
                print("%-40s lse err %.3g (bound %.3g) target err %.3g (bound %.3g)" % (
                    what, abs(lse[0] - want_lse), logprobs_ref.bound(x), abs(tlp[0] - all_lp[target]), logprobs_ref.bound(x, x[target])))
            assert np.array_equal(ids, rids), "%s: ids %s, reference %s" % (what, ids, rids)
            assert logprobs_ref.within(lse, [want_lse], logprobs_ref.bound(x)), "%s: lse %r, reference %r" % (what, lse[0], want_lse)
            assert logprobs_ref.within(top, rlp, logprobs_ref.bound(x, x[rids])), "%s: top log-probabilities %s, reference %s" % (what, top, rlp)
            assert logprobs_ref.within(tlp, [all_lp[target]], logprobs_ref.bound(x, x[target])), "%s: target %r, reference %r" % (what, tlp[0], all_lp[target])
            if name == "all equal":
                assert ids.tolist() == list(range(lo, lo + k))
                if not lo:
                    assert logprobs_ref.within(top, np.full(k, -np.log(n)), logprobs_ref.bound(x))
            if lo:
                assert target >= lo and int(np.argmax(x.astype(np.float32))) >= lo and (k == 0 or rids.min() >= lo), what
                with np.errstate(invalid="ignore"):
                    assert np.flatnonzero(x.astype(np.float32) == x.astype(np.float32).max()).min() >= lo, what
                highest = max(highest, target, int(rids.max()) if k else 0)
            again = _launch(q4, x, k, target)
            for a, b in zip((lse, tlp, ids, top), again):
                assert a.tobytes() == b.tobytes(), what + ": a second launch gave other bits"
    assert not lo or highest > 98304, highest


def test_kernel_without_a_target_and_argument_checks(q4):
    L = q4.lib()
    x = np.linspace(-2, 2, 50).astype(np.float16)
    lse, tlp, ids, top = _launch(q4, x, 3, -1)
    assert np.isnan(tlp[0]) and ids.tolist() == [49, 48, 47]
    lse2, tlp2, _, _ = _launch(q4, x, 0, 50)                    # out of range: no target either
    assert np.isnan(tlp2[0]) and lse2.tobytes() == lse.tobytes()
    d = q4.DevBuf(x)
    o = [q4.DevBuf(nbytes=128) for _ in range(4)]
    assert L.q4_logprob_topk(d.ptr, 8, 9, None, o[0].ptr, o[1].ptr, o[2].ptr, o[3].ptr) == ERR_ARG       # top_k > n
    assert L.q4_logprob_topk(d.ptr, 50, 21, None, o[0].ptr, o[1].ptr, o[2].ptr, o[3].ptr) == ERR_ARG
    assert L.q4_logprob_topk(d.ptr, 0, 0, None, o[0].ptr, o[1].ptr, o[2].ptr, o[3].ptr) == ERR_ARG
    nan = x.copy()
    nan[7] = np.nan                                             # no fault, ids in range, the NaN ranks behind everything
    _, _, ids, _ = _launch(q4, nan, 20, 0)
    assert ids.min() >= 0 and ids.max() < 50 and 7 not in ids.tolist()


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. - 4. inside the decode step
@pytest.fixture(scope="module")
def paths(tmp_path_factory):
    d = tmp_path_factory.mktemp("lp")
    out = {}
    for name in ("small", "tiny_gqa", "v32k", "v40k"):
        out[name] = str(d / (name + ".bin"))
        synth.write_model(out[name], name, seed=7)
    return out


def _sampler(mode):
    return dict(temperature=SAMPLED[0], topp=SAMPLED[1], seed=4242) if mode == "sampled" else dict(temperature=0.0)


def _generate(q4, path, mode, k, prompt=PROMPT, steps=STEPS):
    """one generate_ids run on a fresh model: tokens, the final logits' bits, graphs captured, records (k >= 0)"""
    L = q4.lib()
    t = q4.Transformer(path, logprobs=5 if k == "toggled" else None if k < 0 else k, **_sampler(mode))
    if k == "toggled":           # on, then off again before the first step
        t.set_logprobs(None)
        k = -1
    c0 = L.q4_graph_captures()
    toks = t.generate_ids(prompt, steps)[0].copy()
    res = dict(tokens=toks, logits=t.logits(), captures=L.q4_graph_captures() - c0)
    if k >= 0:
        res["records"] = t.logprobs(0, len(toks) - 1)
    t.close()
    return res


def _replay_logits(q4, path, tokens):
    """the sequence again, one step at a time with records off: the fp16 logits of every position"""
    t = q4.Transformer(path)
    t.reset(tokens)
    out = []
    for pos in range(len(tokens) - 1):
        t.run_transformer_at(pos, 0)
        out.append(t.logits())
    t.close()
    return np.stack(out)


def _check_records(tokens, logits, records, k, n_prompt, greedy, what):
    """every record against the reference over that position's logits; returns how many chosen tokens lay outside the top k"""
    tlp, ids, top = records
    outside = 0
    for p in range(len(tokens) - 1):
        x = logits[p]
        rids, rlp = logprobs_ref.topk(x, k)
        w = "%s, record %d" % (what, p)
        assert np.array_equal(ids[p], rids), "%s: ids %s, reference %s" % (w, ids[p], rids)
        assert logprobs_ref.within(top[p], rlp, logprobs_ref.bound(x, x[rids])), "%s: %s, reference %s" % (w, top[p], rlp)
        tok = int(tokens[p + 1])
        want = logprobs_ref.logprobs(x)[tok]
        assert logprobs_ref.within([tlp[p]], [want], logprobs_ref.bound(x, x[tok])), "%s: token_logprob %r of token %d, reference %r" % (w, tlp[p], tok, want)
        if p >= n_prompt - 1 and greedy:
            assert tok == int(logprobs_ref.topk(x, 1)[0][0]), w
            if k > 0:
                assert ids[p][0] == tok and tlp[p].tobytes() == top[p][0].tobytes(), w
        if k > 0 and tok not in ids[p].tolist():
            outside += 1
    return outside


@pytest.fixture(scope="module")
def runs(q4, paths):
    """the generate runs of items 2 and 3, once: (model, mode) -> {k: result}, plus the stepwise logits of the (common) token sequence"""
    out = {}
    for name in ("small", "tiny_gqa"):
        for mode in ("greedy", "sampled"):
            r = {k: _generate(q4, paths[name], mode, k) for k in (-1, 0, 20, "toggled")}
            r["replay"] = _replay_logits(q4, paths[name], r[-1]["tokens"])
            out[(name, mode)] = r
    return out


@pytest.mark.parametrize("mode", ["greedy", "sampled"])
@pytest.mark.parametrize("name", ["small", "tiny_gqa"])
def test_nothing_else_changes(runs, name, mode):
    r = runs[(name, mode)]
    assert len(r[-1]["tokens"]) == STEPS + 1, "the run stopped at an EOS: pick another seed"
    for k in (0, 20):
        assert np.array_equal(r[k]["tokens"], r[-1]["tokens"]), "K = %d changed the tokens" % k
        assert r[k]["logits"].tobytes() == r[-1]["logits"].tobytes(), "K = %d changed the final logits" % k
    # with the option off the call sequence captures what it captured before the option existed: the eight-step prompt group, the
    # single prompt steps 8 and 9, the eight-step generating groups from 10, the single steps from 34 -- four graphs in one bin;
    # and the record launch adds launches to those graphs, not graphs
    # (four today)
    assert r[0]["captures"] == r[-1]["captures"] and r[20]["captures"] == r[-1]["captures"]
    assert r["toggled"]["captures"] == r[-1]["captures"], "a model whose records were switched on and off again captures otherwise than one never touched"
    assert np.array_equal(r["toggled"]["tokens"], r[-1]["tokens"]) and r["toggled"]["logits"].tobytes() == r[-1]["logits"].tobytes()


@pytest.mark.parametrize("mode", ["greedy", "sampled"])
@pytest.mark.parametrize("name", ["small", "tiny_gqa"])
def test_records_are_right(runs, name, mode):
    r = runs[(name, mode)]
    toks = r[-1]["tokens"]
    if mode == "greedy":     # the stepwise replay reproduces the run: its last logits are the run's (a sampled run ends with the sampler's probabilities there)
        assert r["replay"][-1].tobytes() == r[-1]["logits"].tobytes()
    outside = 0
    for k in (0, 20):
        outside += _check_records(toks, r["replay"], r[k]["records"], k, len(PROMPT), mode == "greedy", "%s %s K %d" % (name, mode, k))
    print("%s %s: %d chosen tokens outside the top 20" % (name, mode, outside))
    if mode == "sampled":
        assert outside > 0, "no sampled token outside the top 20: pick another seed"


def _stepwise(q4, t, prompt, steps, teacher=False, logits=None):
    """steps 0 .. steps - 1 one call at a time (the device feeds itself the tokens); teacher: every token given, all prompt steps"""
    t.reset(prompt)
    for pos in range(steps):
        t.run_transformer_at(pos, 0 if teacher else int(pos >= len(prompt) - 1))
        if logits is not None:
            logits.append(t.logits())
    q4.synchronize()
    return np.array([t.token(i) for i in range(steps + 1)], dtype=np.int32)


@pytest.mark.parametrize("mode", ["greedy", "sampled"])
def test_graph_forms_agree(q4, paths, runs, mode):
    """eight steps per replay (the generate run), one step per replay, and the eager launches of q4_set_use_graphs(2): the same bits"""
    L = q4.lib()
    base = runs[("small", mode)]
    try:
        for graphs in (1, 2):
            L.q4_set_use_graphs(graphs)
            t = q4.Transformer(paths["small"], logprobs=20, **_sampler(mode))
            toks = _stepwise(q4, t, PROMPT, STEPS)
            rec = t.logprobs(0, STEPS)
            t.close()
            assert np.array_equal(toks, base[-1]["tokens"]), "use_graphs %d" % graphs
            for a, b, what in zip(rec, base[20]["records"], ("token_logprob", "top_ids", "top_logprobs")):
                assert a.tobytes() == b.tobytes(), "use_graphs %d: %s differs from the eight-steps-per-replay run" % (graphs, what)
    finally:
        L.q4_set_use_graphs(1)


def test_eager_exact_context_and_fusion_levels(q4, paths, runs):
    """q4_set_use_graphs(0) and fusion level 0 launch the records too: right against each mode's own logits, and bit-equal between fusion
    levels 0 and 1 at the positions whose logits are bit-equal there"""
    L = q4.lib()
    toks = runs[("small", "greedy")][-1]["tokens"]
    got = {}
    try:
        for graphs, level in ((0, q4.DEFAULT_FUSION), (1, 0), (1, 1)):
            L.q4_set_use_graphs(graphs)
            L.q4_set_fusion(level)
            t = q4.Transformer(paths["small"], logprobs=20)
            logits = []
            _stepwise(q4, t, toks, STEPS, teacher=True, logits=logits)
            rec = t.logprobs(0, STEPS)
            t.close()
            _check_records(toks, np.stack(logits), rec, 20, len(toks), True, "use_graphs %d fusion %d" % (graphs, level))
            got[(graphs, level)] = (np.stack(logits), rec)
    finally:
        L.q4_set_use_graphs(1)
        L.q4_set_fusion(q4.DEFAULT_FUSION)
    (l0, r0), (l1, r1) = got[(1, 0)], got[(1, 1)]
    same = [p for p in range(STEPS) if l0[p].tobytes() == l1[p].tobytes()]
    print("fusion 0 and 1: %d of %d positions with bit-equal logits" % (len(same), STEPS))
    for p in same:
        for a, b in zip(r0, r1):
            assert a[p].tobytes() == b[p].tobytes(), p


@pytest.mark.parametrize("name", ["v32k", "v40k"])
def test_large_vocabularies_through_the_model(q4, paths, name):
    """vocab 32000: the register path with the sampler's two launches behind it; vocab 40000: the looping path"""
    for mode in ("greedy", "sampled"):
        r = _generate(q4, paths[name], mode, 20, prompt=[1, 5, 9], steps=8)
        toks = r["tokens"]
        assert len(toks) == 9
        logits = _replay_logits(q4, paths[name], toks)
        _check_records(toks, logits, r["records"], 20, 3, mode == "greedy", "%s %s" % (name, mode))


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. scoring
def test_scoring(q4, paths):
    L = q4.lib()
    toks = np.random.default_rng(5).integers(3, 1024, 49).astype(np.int32)
    toks[0] = 1
    tp = q4.Transformer(paths["small"], perplexity=True)
    ppl = tp.perplexity_ids(toks)
    assert tp.logprobs_k() == -1
    s1 = tp.score_ids(toks)
    assert tp.logprobs_k() == -1, "score_ids left the records on"
    assert s1.shape == (48,) and np.isfinite(s1).all()
    got = float(np.exp(-np.mean(s1.astype(np.float64))))
    print("perplexity_ids %.7g, exp(-mean(score_ids)) %.7g" % (ppl, got))
    assert abs(got - ppl) <= 2e-5 * ppl
    tp.close()
    t0 = q4.Transformer(paths["small"], perplexity=False, logprobs=5)
    s0 = t0.score_ids(toks)
    assert s0.tobytes() == s1.tobytes(), "a perplexity = 0 build scores differently"
    assert t0.logprobs_k() == 5, "score_ids changed the setting"
    tlp, ids, top = t0.logprobs(0, 48)                          # ... and with K on, the call left full records behind
    assert tlp.tobytes() == s0.tobytes() and ids.shape == (48, 5)
    # too many targets for the context
    long = np.ones(t0.config.seq_len + 1, dtype=np.int32)
    out = np.zeros(t0.config.seq_len, dtype=np.float32)
    assert L.q4_score_ids(t0.h, t0.sampler, long.ctypes.data, t0.config.seq_len, out.ctypes.data) == ERR_ARG
    t0.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# 7. life cycle
def test_switching_k_on_a_live_model_recaptures(q4, paths, runs):
    L = q4.lib()
    base = runs[("small", "greedy")]
    t = q4.Transformer(paths["small"], logprobs=5)
    toks = t.generate_ids(PROMPT, STEPS)[0].copy()
    _check_records(toks, base["replay"], t.logprobs(0, STEPS), 5, len(PROMPT), True, "K 5")
    c0 = L.q4_graph_captures()
    t.set_logprobs(20)
    assert t.logprobs_k() == 20
    toks = t.generate_ids(PROMPT, STEPS)[0].copy()
    assert L.q4_graph_captures() == c0 + 4, "the graphs with the record launch were not captured again"
    assert np.array_equal(toks, base[-1]["tokens"])
    _check_records(toks, base["replay"], t.logprobs(0, STEPS), 20, len(PROMPT), True, "K 5 -> 20")
    t.set_logprobs(None)                                        # off again: the graphs without the launch, no ring
    assert t.logprobs_k() == -1
    assert L.q4_get_logprobs(t.h, 0, 1, None, None, None) == ERR_ARG
    assert np.array_equal(t.generate_ids(PROMPT, STEPS)[0], base[-1]["tokens"])
    t.close()


def test_two_models_with_different_k_alternate(q4, paths, runs):
    a = q4.Transformer(paths["small"], logprobs=3)
    b = q4.Transformer(paths["tiny_gqa"], logprobs=7, **_sampler("sampled"))
    for turn in range(2):
        ta = a.generate_ids(PROMPT, STEPS)[0].copy()
        if turn == 0:            # (a reused Sampler continues its coin stream: the second sampled run is another sequence)
            tb = b.generate_ids(PROMPT, STEPS)[0].copy()
            assert np.array_equal(tb, runs[("tiny_gqa", "sampled")][-1]["tokens"])
            rb = b.logprobs(0, STEPS)
        else:
            b.generate_ids(PROMPT, STEPS)
        assert np.array_equal(ta, runs[("small", "greedy")][-1]["tokens"])
        _check_records(ta, runs[("small", "greedy")]["replay"], a.logprobs(0, STEPS), 3, len(PROMPT), True, "model a, turn %d" % turn)
    _check_records(tb, runs[("tiny_gqa", "sampled")]["replay"], rb, 7, len(PROMPT), False, "model b")
    assert a.logprobs(0, 2)[1].shape == (2, 3) and b.logprobs(0, 2)[1].shape == (2, 7)
    a.close()
    b.close()


def test_positions_out_of_range_and_rebuild(q4, paths):
    L = q4.lib()
    for _ in range(2):           # free and rebuild
        t = q4.Transformer(paths["tiny_gqa"], logprobs=2)
        s = t.config.seq_len
        buf = np.zeros(4, dtype=np.float32)
        assert L.q4_get_logprobs(t.h, s, 1, buf.ctypes.data, None, None) == ERR_ARG
        assert L.q4_get_logprobs(t.h, s - 1, 2, buf.ctypes.data, None, None) == ERR_ARG
        assert L.q4_get_logprobs(t.h, -1, 1, buf.ctypes.data, None, None) == ERR_ARG
        assert L.q4_get_logprobs(t.h, s - 1, 1, buf.ctypes.data, None, None) == 0
        assert L.q4_set_logprobs(t.h, 21) == ERR_ARG and t.logprobs_k() == 2
        toks = t.generate_ids([1, 4], 12)[0]
        assert len(toks) >= 2 and np.isfinite(t.logprobs(0, len(toks) - 1)[0]).all()
        t.close()
