"""Log-probability records inside prompt passes and verify passes, and scoring by passes (q4_set_pass_logprobs, q4_logprob_topk_rows; DESIGN.md 3.4 /
3.7 / 3.8, "With records"). A pass computes at every position the logits the per-token step computes, and the row form of the record launch runs the
step's instruction stream per row, so "equal" below always means BYTE-equal against the same library with the switch off (or with passes and
speculation off) on a fresh Transformer: the stepwise run. No tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

import pass_context_ref
import spec_ref
import test_speculative_gpu as tsg                      # the forced drafters (oracle, first wrong, alternating) and the Sampler's random state
from llama_cu_awq_amd import synth
from test_prompt_ingest_gpu import _expected_passes

pytestmark = pytest.mark.gpu

SEED = 11             # of the synthetic checkpoints (the other pass tests': their off runs meet no EOS)
T = 8
GEN = 6               # generated steps behind a prompt
N_PROMPT = 17
STEPS = 150
SAMPLED = dict(temperature=0.8, topp=0.9, seed=7)


@pytest.fixture(scope="module")
def models(tmp_path_factory):
    d = tmp_path_factory.mktemp("pass_logprobs")
    out = {}
    for name in ("ffn_pair7b", "ffn_pair_ragged", "spec_cls_ragged", "pass_long", "tiny"):
        p = str(d / (name + ".bin"))
        synth.write_model(p, name, seed=SEED)
        out[name] = p
    return out


def _prompt(n, seed=5):
    r = np.random.default_rng(seed)
    return [1] + [int(x) for x in r.integers(3, 512, size=n - 1)]       # no EOS (2) inside


def _kv(t, n_pos):
    return np.stack([np.concatenate([np.concatenate(t.kv_row(l, pos)) for l in range(t.config.n_layers)]) for pos in range(n_pos)]).view(np.uint16).copy()


def _records(t, n):
    """records [0, n) as bytes: token_logprob, top_ids, top_logprobs"""
    return tuple(a.tobytes() for a in t.logprobs(0, n))


def _assert_same(a, b, what, keys=("tokens", "kv", "logits", "records")):
    for key in keys:
        x, y = a[key], b[key]
        if key == "records":
            for part, p, q in zip(("token_logprob", "top_ids", "top_logprobs"), x, y):
                assert p == q, "%s: records differ in %s" % (what, part)
        else:
            assert x.shape == y.shape and np.array_equal(x, y), "%s: %s differ" % (what, key)


# ---- 1. the row form of the record launch against the one-block launch, row by row -------------------------------------------------------------
KINDS = ("random", "all -inf", "NaNs", "zeros across rank k", "one +inf")


def _row(rng, kind, n, k):
    x = (rng.standard_normal(n) * 3.0).astype(np.float16)
    if kind == "all -inf":
        x[:] = -np.inf
    elif kind == "NaNs":
        x[rng.choice(n, size=max(1, n // 7), replace=False)] = np.nan
    elif kind == "zeros across rank k":                   # a few positive entries, +0 and -0 on more than k + 1 of the rest, everything else negative
        x = (-np.abs(x) - np.float16(1.0)).astype(np.float16)
        idx = rng.permutation(n)
        pos = max(0, min(k // 2, n - 4))
        x[idx[:pos]] = np.float16(2.0)
        zeros = idx[pos:pos + min(n - pos, k + 6)]
        x[zeros[0::2]] = np.float16(0.0)
        x[zeros[1::2]] = np.float16(-0.0)
    elif kind == "one +inf":
        x[int(rng.integers(n))] = np.inf
    return x


HIGH = 65536          # a vocabulary beyond 16 bits of token id


def _row_beyond_16_bits(rng, kind, n, k):
    """_row on the ids HIGH .. n - 1; below them the same scale 40 down (all -inf: NaN, which ranks behind everything), so the maximum, its ties and the
    top k ids all lie at ids >= HIGH"""
    x = ((rng.standard_normal(n) * 3.0).astype(np.float32) - 40.0).astype(np.float16)
    if kind == "all -inf":
        x[:] = np.nan
    x[HIGH:] = _row(rng, kind, n - HIGH, k)
    return x


def _one(q4, row, k, target):
    """q4_logprob_topk on one contiguous row: the bytes of lse, target_logprob, top_ids, top_logprobs"""
    n = row.shape[0]
    d, dt = q4.DevBuf(row), q4.DevBuf(np.array([target], dtype=np.int32))
    lse, tlp, ids, top = q4.DevBuf(nbytes=4), q4.DevBuf(nbytes=4), q4.DevBuf(nbytes=4 * max(k, 1)), q4.DevBuf(nbytes=4 * max(k, 1))
    q4.logprob_topk(d, n, k, dt, lse, tlp, ids, top)
    q4.synchronize()
    out = (lse.get(np.uint32, 1), tlp.get(np.uint32, 1), ids.get(np.int32, max(k, 1))[:k], top.get(np.uint32, max(k, 1))[:k])
    for b in (d, dt, lse, tlp, ids, top):
        b.free()
    return out


def _rows(q4, x, n, k, targets):
    """q4_logprob_topk_rows on the rows of x ([n_rows][ld]): the same four as arrays by row, and the logits buffer as it is afterwards"""
    n_rows, ld = x.shape
    d = q4.DevBuf(x)
    dt = q4.DevBuf(np.asarray(targets, dtype=np.int32)) if targets is not None else None
    lse, tlp = q4.DevBuf(nbytes=4 * n_rows), q4.DevBuf(nbytes=4 * n_rows)
    ids, top = q4.DevBuf(nbytes=4 * n_rows * max(k, 1)), q4.DevBuf(nbytes=4 * n_rows * max(k, 1))
    q4.logprob_topk_rows(d, ld, n, n_rows, k, dt, lse, tlp, ids, top)
    q4.synchronize()
    out = (lse.get(np.uint32, n_rows), tlp.get(np.uint32, n_rows), ids.get(np.int32, n_rows * max(k, 1))[:n_rows * k].reshape(n_rows, k),
           top.get(np.uint32, n_rows * max(k, 1))[:n_rows * k].reshape(n_rows, k), d.get(np.uint16, n_rows * ld).reshape(n_rows, ld))
    for b in (d, dt, lse, tlp, ids, top):
        if b is not None:
            b.free()
    return out


# n: 8 (one chunk), 513 (ld 520: the tail element), 32000, 32768 (the register path's limit), 40000 (the looping path), 128256 (Llama-3's vocabulary: sixteen
# loop runs, ids beyond 16 bits); ld: n rounded up to 8, and that + 64
SIZES = [(8, 8), (8, 72), (513, 520), (513, 584), (32000, 32000), (32000, 32064), (32768, 32768), (32768, 32832), (40000, 40000), (40000, 40064),
         (128256, 128256), (128256, 128320)]


@pytest.mark.parametrize("n_rows,top_k", [(1, 1), (3, 0), (3, 20), (8, 20), (8, 1)])
@pytest.mark.parametrize("n,ld", SIZES)
def test_rows_equal_the_one_block_launch(q4, n, ld, n_rows, top_k):
    k = min(top_k, n)
    rng = np.random.default_rng(100 * n + 10 * n_rows + k + ld)
    shift = (n + ld + n_rows + k) % len(KINDS)            # which kinds the rows of this case hold: all five at 8 rows, a rotating window else
    kinds = [KINDS[(r + shift) % len(KINDS)] for r in range(n_rows)]
    x = np.empty((n_rows, ld), dtype=np.float16)
    pad = np.where(np.arange(ld - n) % 2 == 0, np.float16(np.nan), np.float16(np.inf)).astype(np.float16)
    lo = HIGH if n > HIGH else 0                          # there every id that decides a record lies beyond 16 bits: asserted on the one-block launch's answer
    for r in range(n_rows):
        x[r, :n] = _row_beyond_16_bits(rng, kinds[r], n, k) if lo else _row(rng, kinds[r], n, k)
        x[r, n:] = pad                                    # NaN and +inf between n and ld: never read, never written
    targets = [(100003 if lo else int(rng.integers(n)), -1, n, int(rng.integers(lo, n)), n + 5, lo, n - 1, -7)[r] for r in range(n_rows)]
    highest = 0
    lse, tlp, ids, top, after = _rows(q4, x, n, k, targets)
    assert after.tobytes() == x.view(np.uint16).tobytes(), "the logits (padding included) were written"
    for r in range(n_rows):
        want = _one(q4, np.ascontiguousarray(x[r, :n]), k, targets[r])
        what = "n %d ld %d rows %d k %d, row %d (%s)" % (n, ld, n_rows, k, r, kinds[r])
        for name, got, ref in zip(("lse", "target_logprob", "top_ids", "top_logprobs"), (lse[r:r + 1], tlp[r:r + 1], ids[r], top[r]), want):
            assert got.tobytes() == ref.tobytes(), "%s: %s %s, the one-block launch %s" % (what, name, got, ref)
        if not 0 <= targets[r] < n:
            assert np.isnan(tlp[r:r + 1].view(np.float32)[0]), what + ": a target outside [0, n) gives NaN"
        if k:
            assert ids[r].min() >= 0 and ids[r].max() < n, what
        if lo:
            ref_ids = want[2]
            assert k == 0 or ref_ids.min() >= lo, "%s: a record id below 65536: %s" % (what, ref_ids)
            with np.errstate(invalid="ignore"):
                row = x[r, :n].astype(np.float32)
                assert np.isnan(row).all() or np.flatnonzero(row == np.nanmax(row)).min() >= lo, what
            highest = max(highest, int(ref_ids.max()) if k else 0, targets[r] if 0 <= targets[r] < n else 0)
    assert not lo or highest > 98304, highest


def test_rows_do_not_see_each_other(q4):
    """permuting the rows permutes the outputs; no targets (NULL) gives NaN everywhere and the same lse"""
    n, ld, k = 513, 584, 20
    rng = np.random.default_rng(77)
    x = np.full((8, ld), np.float16(np.inf), dtype=np.float16)
    for r in range(8):
        x[r, :n] = _row(rng, KINDS[r % len(KINDS)], n, k)
    targets = [int(v) for v in rng.integers(n, size=8)]
    base = _rows(q4, x, n, k, targets)
    perm = rng.permutation(8)
    moved = _rows(q4, x[perm], n, k, [targets[i] for i in perm])
    for name, a, b in zip(("lse", "target_logprob", "top_ids", "top_logprobs"), base[:4], moved[:4]):
        assert a[perm].tobytes() == b.tobytes(), name
    none = _rows(q4, x, n, k, None)
    assert none[0].tobytes() == base[0].tobytes() and np.isnan(none[1].view(np.float32)).all()
    assert none[2].tobytes() == base[2].tobytes() and none[3].tobytes() == base[3].tobytes()
    sub = _rows(q4, x[:3], n, k, targets[:3])             # fewer rows: the same records for those rows
    for a, b in zip(base[:4], sub[:4]):
        assert a[:3].tobytes() == b.tobytes()


# ---- 2. prompt passes with records ---------------------------------------------------------------------------------------------------------------
def _generate(q4, path, on, graphs, prompt, k, bound=256):
    """One generation of len(prompt) + GEN steps on a fresh Transformer with records on: tokens, K / V rows of the prompt positions, final logits,
    records [0, len(prompt) + 5), prompt passes run"""
    L = q4.lib()
    L.q4_set_use_graphs(graphs)
    q4.set_pass_context(bound)
    t = q4.Transformer(path, logprobs=k, pass_logprobs=on)
    try:
        assert t.pass_logprobs() == on and t.logprobs_k() == k
        before = q4.prompt_passes()
        out = {"tokens": t.generate_ids(prompt, len(prompt) + GEN)[0].copy()}
        out["passes"] = q4.prompt_passes() - before
        q4.check(L.q4_handoff_status(t.state))
        out.update(kv=_kv(t, len(prompt)), logits=t.logits().view(np.uint16).copy(), records=_records(t, len(prompt) + 5))
    finally:
        t.close()
        L.q4_set_use_graphs(1)
        q4.set_pass_context(256)
    return out


_OFF = {}


def _off(q4, models, name, graphs, n_prompt, k, bound=256):
    """the stepwise run (switch off: records keep the steps), computed once per case and shared"""
    key = (name, graphs, n_prompt, k, bound)
    if key not in _OFF:
        _OFF[key] = _generate(q4, models[name], False, graphs, _prompt(n_prompt), k, bound)
        assert _OFF[key]["passes"] == 0
    return _OFF[key]


@pytest.mark.parametrize("graphs", [1, 2])
@pytest.mark.parametrize("k", [0, 5])
@pytest.mark.parametrize("n_prompt", [3, 9, 17, 140])
@pytest.mark.parametrize("name", ["ffn_pair7b", "ffn_pair_ragged"])
def test_prompt_passes(q4, models, name, n_prompt, k, graphs):
    off = _off(q4, models, name, graphs, n_prompt, k)
    on = _generate(q4, models[name], True, graphs, _prompt(n_prompt), k)
    assert on["passes"] == _expected_passes(n_prompt) > 0
    _assert_same(off, on, "%s, %d prompt tokens, K %d, graphs %d" % (name, n_prompt, k, graphs))


def test_prompt_passes_strips_classifier(q4, models):
    """vocabulary 16600: the step's classifier is the strips launch with a ragged row split"""
    off = _off(q4, models, "spec_cls_ragged", 1, 17, 5)
    on = _generate(q4, models["spec_cls_ragged"], True, 1, _prompt(17), 5)
    assert on["passes"] == _expected_passes(17) == 2
    _assert_same(off, on, "spec_cls_ragged")


def test_prompt_passes_across_256(q4, models):
    """q4_set_pass_context(2304) and 270 prompt tokens: split-context passes behind position 255 carry records too"""
    off = _off(q4, models, "pass_long", 1, 270, 5, 2304)
    on = _generate(q4, models["pass_long"], True, 1, _prompt(270), 5, 2304)
    want = pass_context_ref.prompt_passes(270, 270 + GEN, 2304, 2304)
    assert on["passes"] == len(want) and any(p[0] >= 256 for p in want)
    _assert_same(off, on, "pass_long, 270 prompt tokens")


# ---- 3. verify passes with records ---------------------------------------------------------------------------------------------------------------
def _spec_run(q4, path, k, on, drafter=None, steps=STEPS, prompt=None, **kw):
    """One generation on a fresh Transformer with records on; on: the switch and speculation (draft 7) with the forced drafter"""
    L = q4.lib()
    prompt = _prompt(N_PROMPT) if prompt is None else prompt
    t = q4.Transformer(path, logprobs=k, pass_logprobs=on, **kw)
    try:
        if on:
            t.set_speculative(draft=7, ngram=3, min=1, sampled=kw.get("temperature", 0.0) != 0.0)
            t.set_drafter(drafter)
        before = q4.prompt_passes()
        out = {"tokens": t.generate_ids(prompt, steps)[0].copy()}
        out["prompt_passes"] = q4.prompt_passes() - before
        q4.check(L.q4_handoff_status(t.state))
        n_pos = t.pos()                                   # (the device position: behind a context shift it lies below the step count)
        assert n_pos == min(steps, len(out["tokens"]) - 1) or t.context_shift()[1] > 0
        out.update(kv=_kv(t, n_pos), logits=t.logits().view(np.uint16).copy(), records=_records(t, n_pos), stats=t.spec_stats(), rng=tsg._rng_state(t))
        L.q4_steps_that_fit.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        cfg = C.cast(L.q4_transformer_config(t.h), C.c_void_p)
        out["groups"] = {pos: L.q4_steps_that_fit(pos, len(prompt), steps, cfg, t.sampler) for pos in range(len(prompt) - 1, steps)}
    finally:
        t.close()
    return out


_SPEC_OFF = {}


def _spec_off(q4, models, k, sampled):
    key = (k, sampled)
    if key not in _SPEC_OFF:
        _SPEC_OFF[key] = _spec_run(q4, models["ffn_pair7b"], k, False, **(SAMPLED if sampled else {}))
        assert _SPEC_OFF[key]["stats"] == (0, 0, 0) and _SPEC_OFF[key]["prompt_passes"] == 0
        assert 2 not in _SPEC_OFF[key]["tokens"][1:].tolist(), "the off run meets an EOS: choose another seed"
    return _SPEC_OFF[key]


@pytest.mark.parametrize("kind", ["oracle", "wrong", "alternating"])
@pytest.mark.parametrize("k", [0, 5])
@pytest.mark.parametrize("sampled", [False, True], ids=["greedy", "sampled"])
def test_verify_passes(q4, models, sampled, k, kind):
    """tokens, K / V rows below the final position, final logits, records [0, final position), the Sampler's random state: those of the run without
    speculation and without prompt passes; the counters: spec_ref.replay's over that run's own tokens"""
    off = _spec_off(q4, models, k, sampled)
    R = off["tokens"]
    on = _spec_run(q4, models["ffn_pair7b"], k, True, drafter=tsg.DRAFTERS[kind](R), **(SAMPLED if sampled else {}))
    what = "%s, K %d, %s drafter" % ("sampled" if sampled else "greedy", k, kind)
    _assert_same(off, on, what)
    assert on["rng"] == off["rng"], what + ": the Sampler's random state differs"
    want, passes = spec_ref.replay(R, N_PROMPT, STEPS, tsg.DRAFTERS[kind](R), 7, lambda pos: on["groups"][pos])
    assert on["stats"] == want, (on["stats"], want)
    assert want[0] >= 10 and on["prompt_passes"] == _expected_passes(N_PROMPT)
    if kind == "oracle":
        assert want[1] == want[2]
    if kind == "wrong":
        assert want[2] == 0
    if kind == "alternating":
        assert 0 < want[2] < want[1]                      # accepted and rejected drafts


def test_verify_tokens_with_records(q4, models):
    """the primitive at position 30 with seven drafts, the fourth wrong: switch off, Q4_NOT_ADMITTED and nothing moved; switch on, it runs and leaves the
    stepwise records"""
    off = _spec_off(q4, models, 5, False)
    R = off["tokens"]
    t = q4.Transformer(models["ffn_pair7b"], logprobs=5)
    try:
        t.generate_ids(R[:N_PROMPT], 30)
        assert t.pos() == 30 and not t.verify_covers(30, 7)
        drafts = [int(x) for x in R[31:38]]
        drafts[3] = tsg._wrong(drafts[3])
        before, rec = t.spec_stats(), _records(t, 30)
        assert t.verify(drafts) is None and t.pos() == 30 and t.spec_stats() == before and _records(t, 30) == rec
        t.set_pass_logprobs(True)
        assert t.verify_covers(30, 7)
        emitted, acc = t.verify(drafts)
        assert acc == 3 and emitted.tolist() == R[31:35].tolist() and t.pos() == 34
        got = t.logprobs(0, 34)
        for part, a, b in zip(("token_logprob", "top_ids", "top_logprobs"), got, off["records"]):
            n = len(a.tobytes()) // 34
            assert a.tobytes() == b[:34 * n], "records [0, 34) differ in " + part
        t.set_pass_logprobs(False)
        assert not t.verify_covers(34, 1) and t.verify([5]) is None and t.pos() == 34
    finally:
        t.close()


# ---- 4. scoring by passes --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scorers(q4, models):
    """(K, switch) -> a Transformer, built on first use and shared by the token counts"""
    made = {}

    def get(k, on, name="ffn_pair7b"):
        if (k, on, name) not in made:
            made[(k, on, name)] = q4.Transformer(models[name], logprobs=k, pass_logprobs=on)
        return made[(k, on, name)]
    yield get
    for t in made.values():
        t.close()


def _score(q4, t, tokens, k):
    before = q4.prompt_passes()
    lp = t.score_ids(tokens)
    out = {"passes": q4.prompt_passes() - before, "lp": lp.tobytes(), "logits": t.logits().view(np.uint16).copy(), "pos": t.pos(), "k": t.logprobs_k()}
    if k is not None:
        out["records"] = _records(t, len(tokens) - 1)
    return out


@pytest.mark.parametrize("n", [1, 2, 9, 17, 140, 270])
@pytest.mark.parametrize("k", [None, 5])
def test_score_ids(q4, scorers, k, n):
    """n scored tokens (n + 1 ids): 270 runs passes below position 256 and steps above it; 1 and the remainder of 9 and 17 run a step"""
    tokens = _prompt(n + 1, seed=9)
    off = _score(q4, scorers(k, False), tokens, k)
    on = _score(q4, scorers(k, True), tokens, k)
    m = min(n, 256)
    assert off["passes"] == 0 and on["passes"] == m // T + (1 if m % T >= 2 else 0)
    assert on["lp"] == off["lp"] and np.isfinite(np.frombuffer(on["lp"], dtype=np.float32)).all()
    assert np.array_equal(on["logits"], off["logits"]), "RunState::logits differ behind the call"
    assert on["pos"] == off["pos"] == n
    assert on["k"] == off["k"] == (-1 if k is None else k)
    if k is not None:
        assert on["records"] == off["records"]


def test_score_ids_other_geometry(q4, scorers):
    tokens = _prompt(18, seed=9)
    off = _score(q4, scorers(5, False, "tiny"), tokens, 5)
    on = _score(q4, scorers(5, True, "tiny"), tokens, 5)
    assert on["passes"] == 0 and on["lp"] == off["lp"] and on["records"] == off["records"] and np.array_equal(on["logits"], off["logits"])


# ---- 5. what stays on steps with the switch on -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["guide", "top_k", "dry", "adaptive", "fp8", "fusion1", "context_shift"])
def test_stays_on_steps(q4, models, case):
    """The switch lifts the records' exclusion and nothing else. With records, the switch and speculation on: no verify pass and no question to the
    drafter under a guide, top-k, DRY, the adaptive truncation, the FP8 cache, fusion level 1 and -- once the offset is non-zero -- context shift; no
    prompt pass under a guide, the adaptive truncation, the FP8 cache and fusion level 1. Top-k and DRY touch generating steps only and never kept
    prompt passes away (csrc/q4_passes.hip): their prompt passes are those of the same run with records off. A run that shifts takes its passes in
    front of the first shift, where the offset is 0, as it does with records off. Results equal the run with the switch and speculation off."""
    L = q4.lib()
    kw, level, steps, guide = {}, None, 60, None
    if case == "guide":
        guide = q4.Guide(np.zeros((1, 512), dtype=np.uint16))           # one state that allows every token
        kw = dict(guide=guide)
    elif case == "top_k":
        kw = dict(sampling=dict(top_k=5))
    elif case == "dry":
        kw = dict(dry=dict(multiplier=0.8, base=1.75, allowed_length=1, last_n=64))
    elif case == "adaptive":
        kw = dict(adaptive=dict(typical_p=0.9))
    elif case == "fp8":
        kw = dict(kv="fp8")
    elif case == "fusion1":
        level = 1
    else:
        kw, steps = dict(context_shift=(4, 64)), 340                   # seq_len 300: one shift
    calls = []

    def drafter(ring, room):
        calls.append(len(ring))
        return [5] * room
    try:
        if level is not None:
            L.q4_set_fusion(level)
        off = _spec_run(q4, models["ffn_pair7b"], 5, False, steps=steps, **kw)
        on = _spec_run(q4, models["ffn_pair7b"], 5, True, drafter=drafter, steps=steps, **kw)
        plain = None
        if case in ("top_k", "dry"):                                    # the same settings with records off: the admission as it was
            t = q4.Transformer(models["ffn_pair7b"], **kw)
            try:
                before = q4.prompt_passes()
                t.generate_ids(_prompt(N_PROMPT), steps)
                plain = q4.prompt_passes() - before
            finally:
                t.close()
    finally:
        if level is not None:
            L.q4_set_fusion(q4.DEFAULT_FUSION)
        if guide is not None:
            guide.close()
    _assert_same(off, on, case)
    if case == "context_shift":      # the drafter sees pos + 1 tokens at step pos: asked below the pass bound (256) in front of the wall, never behind it
        assert len(on["tokens"]) > 301, "the run did not pass the wall"
        assert calls and max(calls) <= 256 and on["stats"][0] == len(calls) and on["prompt_passes"] == _expected_passes(N_PROMPT)
    else:
        assert on["stats"] == (0, 0, 0) and calls == []
        assert on["prompt_passes"] == (plain if plain is not None else 0)
        assert plain is None or plain == _expected_passes(N_PROMPT)
