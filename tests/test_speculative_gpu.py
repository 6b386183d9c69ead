"""Speculative greedy decoding (csrc/spec_verify.h, q4_set_speculative, q4_verify_tokens). A verify pass computes at every position the
logits the per-token step computes, bit for bit, so "equal" below always means BYTE-equal against a run with the feature off on a fresh Transformer:
tokens, the K / V rows of every layer and position, the final logits, the Sampler's random state. Expected counters come from the restatement in
tests/spec_ref.py applied to the off run's own tokens."""
import ctypes as C

import numpy as np
import pytest

import spec_ref
from llama_cu_awq_amd import synth

pytestmark = pytest.mark.gpu

SEED = 11            # of the synthetic checkpoints (test_loop_builtin_drafter's condition holds for it; see there)
N_PROMPT = 17
STEPS = 150
DIM = 4096


class SamplerStruct(C.Structure):      # include/llama2_q4.h Sampler
    _fields_ = [("vocab_size", C.c_int), ("indices", C.c_void_p), ("scan", C.c_void_p), ("sort", C.c_void_p), ("bytes_scan", C.c_size_t),
                ("bytes_sort", C.c_size_t), ("temperature", C.c_float), ("topp", C.c_float), ("rng_state", C.c_ulonglong)]


def _rng_state(t):
    return C.cast(t.sampler, C.POINTER(SamplerStruct)).contents.rng_state


@pytest.fixture(scope="module")
def models(tmp_path_factory):
    d = tmp_path_factory.mktemp("speculative")
    out = {}
    for name in ("ffn_pair7b", "ffn_pair_ragged", "spec_cls_ragged", "tiny"):
        p = str(d / (name + ".bin"))
        synth.write_model(p, name, seed=SEED)
        out[name] = p
    return out


def _prompt(n=N_PROMPT, seed=5):
    r = np.random.default_rng(seed)
    return [1] + [int(x) for x in r.integers(3, 512, size=n - 1)]       # no EOS (2) inside


def _state(t, n_pos):
    kv = np.stack([np.concatenate([np.concatenate(t.kv_row(l, pos)) for l in range(t.config.n_layers)]) for pos in range(n_pos)])
    return kv.view(np.uint16).copy(), t.logits().view(np.uint16).copy()


def _run(q4, path, graphs=1, prompt=None, steps=STEPS, spec=None, drafter=None, groups=False, **kw):
    """One generation on a fresh Transformer: dict(tokens, kv, logits, stats, rng, groups)"""
    L = q4.lib()
    prompt = _prompt() if prompt is None else prompt
    L.q4_set_use_graphs(graphs)
    t = q4.Transformer(path, **kw)
    try:
        if spec is not None:
            t.set_speculative(**spec)
        if drafter is not None:
            t.set_drafter(drafter)
        out = {"tokens": t.generate_ids(prompt, steps)[0].copy()}
        q4.check(L.q4_handoff_status(t.state))
        n_pos = min(steps, len(out["tokens"]) - 1)
        out["kv"], out["logits"] = _state(t, n_pos)
        out["stats"] = t.spec_stats()
        out["rng"] = _rng_state(t)
        if groups:       # what the loop queues at a generating position without a draft (q4_steps_that_fit: existing host logic, asked of the live model)
            L.q4_steps_that_fit.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
            cfg = C.cast(L.q4_transformer_config(t.h), C.c_void_p)
            out["groups"] = {pos: L.q4_steps_that_fit(pos, len(prompt), steps, cfg, t.sampler) for pos in range(len(prompt) - 1, steps)}
    finally:
        t.close()
        L.q4_set_use_graphs(1)
    return out


def _assert_same(a, b, what, rng=True):
    assert np.array_equal(a["tokens"], b["tokens"]), "%s: token rings differ: %s vs %s" % (what, a["tokens"], b["tokens"])
    assert a["kv"].shape == b["kv"].shape and np.array_equal(a["kv"], b["kv"]), "%s: K / V rows differ at positions %s" % (
        what, np.unique(np.argwhere(a["kv"] != b["kv"])[:, 0])[:8])
    assert np.array_equal(a["logits"], b["logits"]), "%s: final logits differ in %d entries" % (what, int((a["logits"] != b["logits"]).sum()))
    assert not rng or a["rng"] == b["rng"], "%s: the Sampler's random state differs" % what


_OFF = {}


def _off(q4, models, name="ffn_pair7b", graphs=1, steps=STEPS):
    """the per-token run, computed once per case and shared"""
    key = (name, graphs, steps)
    if key not in _OFF:
        _OFF[key] = _run(q4, models[name], graphs, steps=steps, groups=True)
        assert _OFF[key]["stats"] == (0, 0, 0)
    return _OFF[key]


def _wrong(tok):
    w = (int(tok) + 1) % 512
    return w + 1 if w == 2 else w


# ---- 1. the classifier launch ------------------------------------------------------------------------------------------------------------------
_CLS = {}


def _cls_case(q4, vocab):
    """wcls, rms_w, eight rows of x and -- computed once, row by row, with the public ops -- their reference logits"""
    if vocab not in _CLS:
        L = q4.lib()
        r = np.random.default_rng(vocab)
        w = (r.standard_normal((vocab, DIM), dtype=np.float32) * 0.02).astype(np.float16)
        rms = (1.0 + 0.1 * r.uniform(-1, 1, DIM)).astype(np.float16)
        x = r.standard_normal((8, DIM), dtype=np.float32)
        x[1] = 0.0                                                    # an all-zero row
        x[2] = np.sign(x[2]) * (6e4 / np.sqrt(DIM))                   # a row at the top of fp16's range after the norm's sum (magnitude 6e4 / sqrt(dim))
        x[4] *= 30.0
        x[6] *= 1e-3
        x = x.astype(np.float16)
        dw, dr, dx = q4.DevBuf(w), q4.DevBuf(rms), q4.DevBuf(x)
        xn, lo = q4.DevBuf(nbytes=DIM * 2), q4.DevBuf(nbytes=vocab * 2)
        ref = np.empty((8, vocab), dtype=np.uint16)
        for i in range(8):
            q4.check(L.q4_rmsnorm(xn.ptr, dx.ptr + i * DIM * 2, dr.ptr, DIM))
            q4.check(L.q4_matmul_f16(lo.ptr, xn.ptr, dw.ptr, DIM, vocab, 1, 0, 0, 0, -1, 1.0))
            ref[i] = lo.get(np.uint16, vocab)
        _CLS[vocab] = (dw, dr, dx, ref)
    return _CLS[vocab]


@pytest.mark.parametrize("n", [1, 2, 5, 8])
@pytest.mark.parametrize("vocab", [512, 16600])
def test_classifier_rows(q4, vocab, n):
    """Every row of the n-row launch holds the bits q4_rmsnorm + q4_matmul_f16 give for that row alone: vocab 512 is the plain fp16 GEMV, 16600 the strips
    form with a ragged row split (64.8 rows per CU)."""
    dw, dr, dx, ref = _cls_case(q4, vocab)
    out = q4.DevBuf(nbytes=8 * vocab * 2)
    q4.verify_classifier(out, dx, dr, dw, DIM, vocab, n)
    got = out.get(np.uint16, 8 * vocab).reshape(8, vocab)
    for i in range(n):
        bad = np.flatnonzero(got[i] != ref[i])
        assert bad.size == 0, "row %d of %d, vocab %d: %d logits differ, first at %d" % (i, n, vocab, bad.size, bad[0])
    assert not got[n:].any()                                          # rows past n are not written
    assert np.isfinite(ref.view(np.float16).astype(np.float32)).all() and ref[0].any() and not ref[1].any()


def test_classifier_refuses_other_shapes(q4):
    dw, dr, dx, _ = _cls_case(q4, 512)
    out = q4.DevBuf(nbytes=8 * 512 * 2)
    L = q4.lib()
    assert L.q4_verify_classifier(out.ptr, dx.ptr, dr.ptr, dw.ptr, 2048, 512, 2) == 1          # Q4_ERR_UNSUPPORTED_SIZE
    assert L.q4_verify_classifier(out.ptr, dx.ptr, dr.ptr, dw.ptr, DIM, 508, 2) == 1
    assert L.q4_verify_classifier(out.ptr, dx.ptr, dr.ptr, dw.ptr, DIM, 512, 9) == 5           # Q4_ERR_ARG
    assert L.q4_verify_classifier(out.ptr, None, dr.ptr, dw.ptr, DIM, 512, 2) == 5


# ---- 2. the accept launch ----------------------------------------------------------------------------------------------------------------------
def _accept_rows(size):
    """eight crafted rows of `size` fp16 logits"""
    r = np.random.default_rng(size)
    rows = (r.uniform(-4, 4, (8, size))).astype(np.float16)
    rows[0, 0] = rows[0, size - 1] = 9.0                              # a tie between the first index and the last (the tail loop's): the first wins
    if size > 1024:
        rows[1, 700] = rows[1, 300] = rows[1, size - 2] = 8.5         # a tie across waves (thread u owns chunk u: elements 0 .. 511 are wave 0's) and the tail
    else:
        rows[1, 100] = rows[1, size - 1] = 8.5                        # ... between a chunk and the tail
    rows[2, :] = -np.inf                                              # no candidate: 0
    rows[3, :] = np.nan                                               # the same
    rows[4, ::3] = np.nan                                             # NaNs never win
    rows[4, 1] = -np.inf
    rows[5, 7] = rows[5, 8] = np.float16(6.0)                         # a tie across two chunks of one wave
    rows[6, size - 3] = 7.0                                           # the winner in the tail
    return rows


@pytest.mark.parametrize("match", [0, 1, 3, 6, 7])
@pytest.mark.parametrize("size", [517, 1101])
def test_accept(q4, size, match):
    """Crafted logits, sizes that are no multiple of 8 (the tail loop runs; 1101 spreads a row over three waves): the rows' tokens, m, the ring, the
    position words and the copies of row m against the numpy restatement, for drafts that match 0, some and all rows."""
    rows = _accept_rows(size)
    ld = (size + 7) // 8 * 8
    D, p, dim = 7, 40, 64
    win, _ = spec_ref.accept(rows, [])
    assert win[0] == 0 and win[1] == (300 if size > 1024 else 100) and win[2] == 0 and win[3] == 0 and win[5] == 7 and win[6] == size - 3
    drafts = [win[i] if i < match else _wrong(win[i]) for i in range(D)]
    _, m = spec_ref.accept(rows, drafts)
    assert m == match
    padded = np.zeros((8, ld), dtype=np.float16)
    padded[:, :size] = rows
    padded[:, size:] = 60000.0                                        # the padding behind a row is never read
    x = np.random.default_rng(3).standard_normal((8, dim)).astype(np.float16)
    dl, dx = q4.DevBuf(padded), q4.DevBuf(x)
    lo, xo = q4.DevBuf(nbytes=ld * 2), q4.DevBuf(nbytes=dim * 2)
    ring = q4.DevBuf(np.full(64, -7, dtype=np.int32))
    ph, pd = q4.DevBuf(np.array([p], dtype=np.int32)), q4.DevBuf(np.array([p], dtype=np.int32))
    rep = q4.DevBuf(np.full(9, -3, dtype=np.int32))
    q4.verify_accept(dl, ld, size, drafts, dx, dim, lo, xo, ring, ph, pd, rep)
    q4.synchronize()
    assert rep.get(np.int32, 9).tolist() == win + [m]
    got_ring = ring.get(np.int32, 64)
    assert got_ring[p + 1:p + m + 2].tolist() == win[:m + 1]
    assert (got_ring[:p + 1] == -7).all() and (got_ring[p + m + 2:] == -7).all()
    assert ph.get(np.int32, 1)[0] == p + m + 1 and pd.get(np.int32, 1)[0] == p + m + 1
    assert np.array_equal(lo.get(np.uint16, size), rows[m].view(np.uint16))
    assert not lo.get(np.uint16, ld)[size:].any()
    assert np.array_equal(xo.get(np.uint16, dim), x[m].view(np.uint16))


def test_accept_refuses_bad_arguments(q4):
    L = q4.lib()
    b = q4.DevBuf(nbytes=4096)
    d = (C.c_int * 8)(*range(8))
    args = lambda ld, size, nd: (b.ptr, ld, size, d, nd, None, 64, b.ptr, None, b.ptr, b.ptr, b.ptr, None)
    assert L.q4_verify_accept(*args(520, 517, 0)) == 5 and L.q4_verify_accept(*args(520, 517, 8)) == 5
    assert L.q4_verify_accept(*args(517, 517, 3)) == 5 and L.q4_verify_accept(*args(512, 517, 3)) == 5


# ---- 3. the primitive --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def stepwise(q4, models):
    """R: the per-token greedy run of the 17-token prompt to 150 steps through the per-step entry point, with the logits behind every step"""
    q4.lib().q4_set_use_graphs(1)
    t = q4.Transformer(models["ffn_pair7b"])
    prompt = _prompt()
    t.reset(prompt)
    logits = []
    for pos in range(STEPS):
        t.run_transformer_at(pos, pos >= N_PROMPT - 1)
        logits.append(t.logits().view(np.uint16).copy())
    q4.synchronize()
    ring = np.array([t.token(i) for i in range(STEPS + 1)], dtype=np.int32)
    kv, _ = _state(t, STEPS)
    assert t.speculative()["draft"] == 0 and t.spec_stats() == (0, 0, 0)          # off unless asked for
    yield {"t": t, "ring": ring, "logits": logits, "kv": kv}
    t.close()


def test_default_is_off(q4, stepwise):
    assert stepwise["t"].speculative() == {"draft": 0, "ngram": 0, "min": 0}


@pytest.mark.parametrize("D", [1, 3, 7])
@pytest.mark.parametrize("p", [16, 60, 123, 126])
def test_primitive(q4, stepwise, p, D):
    """q4_verify_tokens at position p with D drafts whose first wrong index k takes every value 0 .. D (p = 123 and 126 straddle the 128 bin inside a
    pass): n_accepted, the emitted tokens, the position and the logits there; then per-token steps to 150 over the rows the pass left."""
    t, R = stepwise["t"], stepwise["ring"]
    for k in range(D + 1):
        t.generate_ids(R[:N_PROMPT], p)                               # per-token (and prompt passes) to position p: ring[p] is R's
        assert t.pos() == p and t.verify_covers(p, D)
        drafts = [int(R[p + 1 + i]) for i in range(D)]
        if k < D:
            drafts[k] = _wrong(R[p + 1 + k])
        before = t.spec_stats()
        emitted, acc = t.verify(drafts)
        assert acc == k, "p %d, D %d, first wrong %d: accepted %d" % (p, D, k, acc)
        assert emitted.tolist() == R[p + 1:p + k + 2].tolist()
        assert t.pos() == p + k + 1
        assert np.array_equal(t.logits().view(np.uint16), stepwise["logits"][p + k]), "logits behind the pass (p %d, D %d, k %d)" % (p, D, k)
        after = t.spec_stats()
        assert (after[0] - before[0], after[1] - before[1], after[2] - before[2]) == (1, D, k)
        toks = t.generate_ids_from(R[:p + k + 2], STEPS, p + k + 1)[0]
        assert np.array_equal(toks, R), "ring behind the pass (p %d, D %d, k %d)" % (p, D, k)
        kv, logits = _state(t, STEPS)
        bad = np.unique(np.argwhere(kv != stepwise["kv"])[:, 0])
        assert bad.size == 0, "K / V rows differ at positions %s (p %d, D %d, k %d)" % (bad[:8], p, D, k)
        assert np.array_equal(logits, stepwise["logits"][STEPS - 1])


def test_primitive_arguments_and_admission(q4, stepwise, models):
    t, R = stepwise["t"], stepwise["ring"]
    L = q4.lib()
    t.generate_ids(R[:N_PROMPT], 30)
    out, acc = (C.c_int * 9)(), C.c_int()
    ids = lambda *a: (C.c_int * len(a))(*a)
    for bad, n in ((ids(512), 1), (ids(-1), 1), (ids(5, 600), 2), (ids(*range(8)), 8), (ids(5), 0)):
        assert L.q4_verify_tokens(t.h, bad, n, out, C.byref(acc)) == 5
    assert L.q4_verify_tokens(t.h, None, 1, out, C.byref(acc)) == 5
    assert t.pos() == 30 and t.spec_stats()[0] >= 0
    assert t.verify_covers(248, 7) and not t.verify_covers(249, 7) and t.verify_covers(254, 1) and not t.verify_covers(255, 1)
    # records on: not admitted, nothing runs, the position stays
    t.set_logprobs(0)
    before = t.spec_stats()
    assert t.verify([int(R[31])]) is None and t.pos() == 30 and t.spec_stats() == before
    t.set_logprobs(None)
    assert t.verify([int(R[31])])[1] == 1
    tiny = q4.Transformer(models["tiny"])
    try:
        tiny.generate_ids([1, 20, 300], 8)
        assert not tiny.verify_covers(8, 1) and tiny.verify([5]) is None and tiny.pos() == 8
    finally:
        tiny.close()


# ---- 4. the loop with forced drafters ----------------------------------------------------------------------------------------------------------
def _oracle(R):
    return lambda ring, room: R[len(ring):len(ring) + room]


def _wrong_drafter(R):
    return lambda ring, room: [_wrong(R[len(ring)])] + [int(x) for x in R[len(ring) + 1:len(ring) + room]]


def _alternating(R):
    """by call: everything right, first wrong, second wrong, no draft"""
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


DRAFTERS = {"oracle": _oracle, "wrong": _wrong_drafter, "alternating": _alternating}


@pytest.mark.parametrize("graphs", [1, 2])
@pytest.mark.parametrize("kind", ["oracle", "wrong", "alternating"])
@pytest.mark.parametrize("name", ["ffn_pair7b", "ffn_pair_ragged"])
def test_loop_forced_drafters(q4, models, name, kind, graphs):
    off = _off(q4, models, name, graphs)
    R = off["tokens"]
    on = _run(q4, models[name], graphs, spec=dict(draft=7, ngram=3, min=1), drafter=DRAFTERS[kind](R))
    _assert_same(off, on, "%s, %s drafter, graphs %d" % (name, kind, graphs))
    want, passes = spec_ref.replay(R, N_PROMPT, STEPS, DRAFTERS[kind](R), 7, lambda pos: off["groups"][pos] if graphs == 1 else 1)
    assert on["stats"] == want, (on["stats"], want)
    assert want[0] >= 10
    if kind == "oracle":
        assert want[1] == want[2] and all(p[1] == 7 for p in passes[:-1])       # every pass accepts everything; only the last may be cut by `steps`
    if kind == "wrong":
        assert want[2] == 0


def test_loop_strips_classifier(q4, models):
    """the one-layer model whose classifier is the strips launch with a ragged row split"""
    off = _off(q4, models, "spec_cls_ragged", 1, 80)
    R = off["tokens"]
    on = _run(q4, models["spec_cls_ragged"], 1, steps=80, spec=dict(draft=5, ngram=3, min=1), drafter=_alternating(R))
    _assert_same(off, on, "spec_cls_ragged")
    want, _ = spec_ref.replay(R, N_PROMPT, 80, _alternating(R), 5, lambda pos: off["groups"][pos])
    assert on["stats"] == want and want[0] >= 5 and 0 < want[2] < want[1]


# ---- 5. the loop with the built-in drafter -----------------------------------------------------------------------------------------------------
def test_loop_builtin_drafter(q4, models):
    """n-grams 3 .. 1, 7 drafts, 250 steps. Seed 11's off run must itself contain at least three passes with an accepted draft and one with none
    (the CPU oracle shows 48 passes and 16 accepted drafts for this seed and prompt; the GPU's tokens may drift from it, so the condition is asserted
    on the GPU's own off run)."""
    steps = 250
    off = _off(q4, models, "ffn_pair7b", 1, steps)
    R = off["tokens"]
    builtin = lambda ring, room: spec_ref.draft(ring, room, 3, 1)
    want, passes = spec_ref.replay(R, N_PROMPT, steps, builtin, 7, lambda pos: off["groups"][pos])
    print("built-in drafter over the off run: passes, drafted, accepted = %s; distinct tokens %d" % (want, len(set(R.tolist()))))
    assert sum(1 for p in passes if p[2] > 0) >= 3 and sum(1 for p in passes if p[2] == 0) >= 1, passes
    on = _run(q4, models["ffn_pair7b"], 1, steps=steps, spec=dict(draft=7, ngram=3, min=1))
    _assert_same(off, on, "built-in drafter")
    assert on["stats"] == want, (on["stats"], want)


# ---- 6. not admitted ---------------------------------------------------------------------------------------------------------------------------
def _guide(q4):
    return q4.Guide(np.zeros((1, 512), dtype=np.uint16))               # one state that allows every token


@pytest.mark.parametrize("case", ["temperature", "top_k", "guide", "logprobs", "tiny", "fusion1", "fusion0", "fp8"])
def test_not_admitted_runs_the_steps(q4, models, case):
    L = q4.lib()
    name, kw, level, steps = "ffn_pair7b", {}, None, 60
    if case == "temperature":
        kw = dict(temperature=0.8, topp=0.9, seed=7)
    elif case == "top_k":
        kw = dict(sampling=dict(top_k=5))
    elif case == "guide":
        kw = dict(guide=_guide(q4))
    elif case == "logprobs":
        kw = dict(logprobs=0)
    elif case == "tiny":
        name, steps = "tiny", 40
    elif case == "fp8":
        kw = dict(kv="fp8")
    else:
        level = int(case[-1])
    calls = []

    def drafter(ring, room):
        calls.append(len(ring))
        return [5] * room
    try:
        if level is not None:
            L.q4_set_fusion(level)
        off = _run(q4, models[name], 1, steps=steps, **kw)
        on = _run(q4, models[name], 1, steps=steps, spec=dict(draft=7, ngram=3, min=1), drafter=drafter, **kw)
    finally:
        if level is not None:
            L.q4_set_fusion(q4.DEFAULT_FUSION)
        if "guide" in kw:
            kw["guide"].close()
    assert on["stats"] == (0, 0, 0) and calls == []
    _assert_same(off, on, case)


def test_verifies_only_below_256(q4, models):
    """a generation to 270 positions: passes while every position of a pass is below 256, steps behind"""
    off = _off(q4, models, "ffn_pair7b", 1, 270)
    R = off["tokens"]
    seen = []

    def drafter(ring, room):
        seen.append((len(ring) - 1, room))
        return R[len(ring):len(ring) + room]
    on = _run(q4, models["ffn_pair7b"], 1, steps=270, spec=dict(draft=7, ngram=3, min=1), drafter=drafter)
    _assert_same(off, on, "270 positions")
    want, _ = spec_ref.replay(R, N_PROMPT, 270, _oracle(R), 7, lambda pos: off["groups"][pos])
    assert on["stats"] == want
    assert max(pos + room for pos, room in seen) == 255 and seen[-1][0] < 255


# ---- 7. afterwards -----------------------------------------------------------------------------------------------------------------------------
def test_second_generation_equals_a_fresh_one(q4, models):
    off = _off(q4, models)
    R = off["tokens"]
    second = _prompt(N_PROMPT + 3, seed=21)
    fresh = _run(q4, models["ffn_pair7b"], 1, prompt=second, steps=60)
    L = q4.lib()
    t = q4.Transformer(models["ffn_pair7b"], speculative=dict(draft=7, ngram=3, min=1))
    try:
        assert t.speculative() == {"draft": 7, "ngram": 3, "min": 1}
        t.set_drafter(_alternating(R))
        t.generate_ids(_prompt(), STEPS)
        assert t.spec_stats()[0] > 0
        t.set_drafter(None)
        t.set_speculative(draft=0)
        again = {"tokens": t.generate_ids(second, 60)[0].copy()}
        q4.check(L.q4_handoff_status(t.state))
        again["kv"], again["logits"] = _state(t, 60)
    finally:
        t.close()
    _assert_same(fresh, again, "second generation", rng=False)          # (this Sampler has drawn the first generation's coins too)


def test_common_prefix_behind_rejected_drafts(q4, models):
    """A pass whose drafts are all rejected leaves draft rows above the position: the common prefix stops at the position, and a generation that reuses
    it gives the full run's bytes"""
    off = _off(q4, models)
    R = off["tokens"]
    t = q4.Transformer(models["ffn_pair7b"])
    try:
        t.generate_ids(R[:N_PROMPT], 60)
        emitted, acc = t.verify([_wrong(R[61])] + [int(x) for x in R[62:68]])
        assert acc == 0 and emitted.tolist() == [int(R[61])] and t.pos() == 61
        assert t.common_prefix(R[:100]) == 61
        toks = t.generate_ids(R[:62], STEPS, reuse=True)
        assert toks[2] == STEPS - 1 - 61                             # the steps that ran
        got = {"tokens": toks[0].copy(), "rng": _rng_state(t)}
        got["kv"], got["logits"] = _state(t, STEPS)
    finally:
        t.close()
    _assert_same(off, got, "reused prefix behind a pass", rng=False)     # (this Sampler has drawn the first 60 steps' coins twice)


def test_snapshot_after_a_speculative_run(q4, models):
    off = _off(q4, models)
    R = off["tokens"]
    t = q4.Transformer(models["ffn_pair7b"], speculative=dict(draft=7, ngram=3, min=1))
    t2 = None
    try:
        t.set_drafter(_alternating(R))
        first = t.generate_ids(_prompt(), 100)[0]
        assert np.array_equal(first, R[:101]) and t.spec_stats()[0] > 0
        snap = t.snapshot()
        assert snap.n_pos == 100
        t2 = q4.Transformer(models["ffn_pair7b"])
        toks = t2.generate_ids(R[:101], STEPS, reuse=snap)
        assert toks[2] == STEPS - 1 - 100
        got = {"tokens": toks[0].copy(), "rng": _rng_state(t2)}
        got["kv"], got["logits"] = _state(t2, STEPS)
        snap.close()
    finally:
        t.close()
        if t2 is not None:
            t2.close()
    _assert_same(off, got, "restored snapshot")


# ---- 8. the passes' scratch belongs to its model -----------------------------------------------------------------------------------------------
def test_pass_scratch_lives_and_dies_with_its_model(q4, models):
    """The scratch of prompt and verify passes is part of the model's record (csrc/q4_model.h PassScratch): allocated by the model's first pass, released
    by q4_free_transformer. Model A runs prompt passes and a verify pass and is freed; B, built where A may have lived, runs the same; C is built beside B
    and verify passes alternate between the two, with drafts accepted and rejected. Every run's tokens and the K / V rows below its position are the
    bytes of the per-token steps: the same checkpoint with q4_set_prompt_ingest(0) and no speculation."""
    L = q4.lib()
    path, prompt, p = models["spec_cls_ragged"], _prompt(), 20
    ingest_max = q4.get_prompt_ingest()
    q4.set_prompt_ingest(0)
    ref = q4.Transformer(path)
    try:
        passes = q4.prompt_passes()
        R = ref.generate_ids(prompt, p + 12)[0].copy()
        q4.check(L.q4_handoff_status(ref.state))
        assert q4.prompt_passes() == passes and ref.spec_stats() == (0, 0, 0)
        assert len(R) == p + 13 and 2 not in R[1:].tolist()              # (no EOS: the run reached its last step)
        kv = _state(ref, p + 12)[0]
    finally:
        ref.close()
        q4.set_prompt_ingest(ingest_max)

    def ingest(t, what):          # positions 0 .. 15 in prompt passes, 16 .. p - 1 in steps
        before = q4.prompt_passes()
        toks = t.generate_ids(prompt, p)[0]
        assert q4.prompt_passes() > before, "%s: no prompt pass ran" % what
        assert np.array_equal(toks, R[:p + 1]), "%s: tokens behind the prompt passes" % what
        return p

    def verify(t, pos, k, what):  # a verify pass with 2 drafts, the first k of them right: the position behind it
        assert t.pos() == pos and t.verify_covers(pos, 2), what
        drafts = [int(R[pos + 1]), int(R[pos + 2])]
        if k < 2:
            drafts[k] = _wrong(R[pos + 1 + k])
        before = t.spec_stats()
        emitted, acc = t.verify(drafts)
        assert acc == k and emitted.tolist() == R[pos + 1:pos + k + 2].tolist() and t.pos() == pos + k + 1, "%s: pass at %d, %d right" % (what, pos, k)
        assert t.spec_stats() == (before[0] + 1, before[1] + 2, before[2] + k), what
        bad = np.unique(np.argwhere(_state(t, pos + k + 1)[0] != kv[:pos + k + 1])[:, 0])
        assert bad.size == 0, "%s: K / V rows differ at positions %s behind the pass at %d" % (what, bad[:8], pos)
        return pos + k + 1

    a = q4.Transformer(path)
    try:
        verify(a, ingest(a, "A"), 2, "A")
        q4.check(L.q4_handoff_status(a.state))
    finally:
        a.close()
    b, c = q4.Transformer(path), None
    try:
        pos_b = verify(b, ingest(b, "B, built after A was freed"), 2, "B, built after A was freed")
        c = q4.Transformer(path)
        pos_c = ingest(c, "C beside B")
        for k_b, k_c in ((2, 0), (1, 2), (0, 1)):
            pos_b = verify(b, pos_b, k_b, "B, alternating with C")
            pos_c = verify(c, pos_c, k_c, "C, alternating with B")
        q4.check(L.q4_handoff_status(b.state))
        q4.check(L.q4_handoff_status(c.state))
    finally:
        b.close()
        if c is not None:
            c.close()
