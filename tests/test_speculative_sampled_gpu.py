"""Verify passes under the temperature / top-p sampler (q4_set_speculative_sampled; DESIGN.md 3.8, "Under the sampler"). Every row of a pass is sampled
with its own position's coin exactly as the step samples, so "equal" below always means BYTE-equal against a run with the feature off on a fresh
Transformer with the same temperature, top-p and seed: tokens, the K / V rows of every layer and position, the final logits (the fp16 probabilities the
sampler leaves in place), the Sampler's random state. Expected counters come from tests/spec_ref.py's replay applied to the off run's own tokens; coins
from tests/spec_sampled_ref.py."""
import ctypes as C

import numpy as np
import pytest

import spec_ref
import spec_sampled_ref as ref
from llama_cu_awq_amd import synth

pytestmark = pytest.mark.gpu

SEED = 11            # of the synthetic checkpoints
N_PROMPT = 17
STEPS = 150
TEMP, TOPP, RNG = 0.8, 0.9, 7


@pytest.fixture(scope="module")
def models(tmp_path_factory):
    d = tmp_path_factory.mktemp("speculative_sampled")
    out = {}
    for name in ("ffn_pair7b", "ffn_pair_ragged", "spec_cls_ragged", "tiny", "v32k", "v40k"):
        p = str(d / (name + ".bin"))
        synth.write_model(p, name, seed=SEED)
        out[name] = p
    return out


def _rng_state(t):
    return ref.sampler_struct(t.sampler).rng_state


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


def _off(q4, models, name="ffn_pair7b", graphs=1, steps=STEPS, temperature=TEMP, topp=TOPP, seed=RNG):
    """the per-token sampled run, computed once per case and shared"""
    key = (name, graphs, steps, temperature, topp, seed)
    if key not in _OFF:
        _OFF[key] = _run(q4, models[name], graphs, steps=steps, groups=True, temperature=temperature, topp=topp, seed=seed)
        assert _OFF[key]["stats"] == (0, 0, 0)
        assert 2 not in _OFF[key]["tokens"][1:].tolist(), "the off run meets an EOS: choose another seed"
    return _OFF[key]


def _wrong(tok):
    w = (int(tok) + 1) % 512
    return w + 1 if w == 2 else w


SPEC = dict(draft=7, ngram=3, min=1, sampled=True)


# ---- 1. the row form of the sampler against the step's own sampler -----------------------------------------------------------------------------
TP = [(0.5, 0.6), (1.0, 0.9), (0.8, 1.0), (1.3, 0.0), (0.05, 0.9)]
# One coin per ROW (k / 2^24: the values the sampler's stream can yield): 0.0, 2^-23 (the stream's neighbour of 1e-7), 0.5, 0.99999994, ...
# Row 0 (ordinary) has coin 0.0: its top probability reaches any threshold -- the shortcut. Row 7 (exactly flat, every probability 1 / vocab <= 1 / 512)
# has coin 0.99999994: with p >= 0.6 the threshold is above 0.59 -- never the shortcut. Every case below runs row 0 and row 7.
COIN_K = [0, 2, 1 << 23, (1 << 24) - 1, 5033165, 12582912, 15099494, (1 << 24) - 1]
COINS = [k / 16777216.0 for k in COIN_K]


def _logit_case(rng, vocab, kind):
    """test_sampling_gpu.py's distributions, restated: ordinary, wide, nearly flat, exactly flat, ties at the maximum, few distinct values, one dominant"""
    if kind == 0:
        x = rng.standard_normal(vocab) * 2.0
    elif kind == 1:
        x = rng.standard_normal(vocab) * 6.0
    elif kind == 2:
        x = rng.standard_normal(vocab) * 0.05
    elif kind == 3:
        x = np.full(vocab, float(rng.standard_normal()))
    elif kind == 4:
        x = rng.standard_normal(vocab) * 2.0
        x[rng.integers(0, vocab, 8)] = x.max() + 0.5
    elif kind == 5:
        x = rng.integers(-3, 4, vocab).astype(np.float64)
    else:
        x = rng.standard_normal(vocab)
        x[int(rng.integers(0, vocab))] = 12.0
    return x.astype(np.float16)


def _rows(vocab):
    """eight rows: the seven distributions (the exactly flat one last) and, as row 6, one with a third of its entries -inf"""
    rng = np.random.default_rng(vocab)
    rows = [_logit_case(rng, vocab, kind) for kind in (0, 1, 2, 4, 5, 6)]
    masked = (rng.standard_normal(vocab) * 2.0).astype(np.float16)
    masked[::3] = -np.inf
    rows.append(masked)
    rows.append(_logit_case(rng, vocab, 3))
    return np.stack(rows)


@pytest.fixture(scope="module")
def host(q4, models):
    """a RunState with room for 32000 logits: q4_sample runs on it with samplers of any smaller vocabulary"""
    t = q4.Transformer(models["v32k"])
    yield t
    t.close()


_REF = {}


def _reference(q4, orc, host, vocab, temperature, topp):
    """per row: the token and the in-place probabilities q4_sample leaves for that row alone with the row's coin -- computed once per (vocab, T, p)"""
    key = (vocab, temperature, topp)
    if key not in _REF:
        L = q4.lib()
        rows = _rows(vocab)
        s = L.q4_sampler_new(vocab, temperature, topp, 1)
        assert s
        toks, probs = [], np.empty((8, vocab), dtype=np.uint16)
        try:
            for r in range(8):
                host.reset([1])
                q4.check(L.q4_memcpy_h2d(host.state.contents.logits, rows[r].ctypes.data, rows[r].nbytes))
                ref.sampler_struct(s).rng_state = ref.state_for_coin(COIN_K[r])
                q4.check(L.q4_sample(s, host.state, 1))
                q4.synchronize()
                assert host.pos() == 1
                toks.append(host.token(1))
                q4.check(L.q4_memcpy_d2h(probs[r].ctypes.data, host.state.contents.logits, probs[r].nbytes))
                if np.isfinite(rows[r].astype(np.float32)).all():
                    want = orc.lib().orc_sample_topp(orc.f16_bits(rows[r].copy()), vocab, temperature, topp, COINS[r])
                    assert toks[r] == want, "q4_sample vs the restatement: row %d, vocab %d, T %g, p %g: %d vs %d" % (r, vocab, temperature, topp, toks[r], want)
        finally:
            L.q4_sampler_delete(s)
        _REF[key] = (toks, probs)
    return _REF[key]


@pytest.mark.parametrize("n", [1, 2, 5, 8])
@pytest.mark.parametrize("temperature,topp", TP)
@pytest.mark.parametrize("vocab", [512, 16600, 32000])
def test_row_sampler(q4, orc, host, vocab, temperature, topp, n):
    """n rows per launch -- rows 0 .. n - 1, and rows 8 - n .. 7 -- with vocabularies of one key per thread (512), a ragged E = 17 (16600) and the
    in-register E = 32 paths (32000): each row's token and all of its in-place probabilities equal q4_sample's for that row alone with that coin; rows
    outside the launch and the padding behind every row stay as they were; with top-p inside (0, 1) both the shortcut and the search occur."""
    L = q4.lib()
    rows = _rows(vocab)
    toks, probs = _reference(q4, orc, host, vocab, temperature, topp)
    ld = vocab + 24
    PAD = np.float16(60000.0).view(np.uint16)
    s = L.q4_sampler_new(vocab, temperature, topp, 1)
    assert s
    took = []
    try:
        for first in sorted({0, 8 - n}):
            padded = np.full((8, ld), PAD, dtype=np.uint16)
            padded[:, :vocab] = rows.view(np.uint16)
            buf = q4.DevBuf(padded)
            out = q4.DevBuf(np.full(8, -9, dtype=np.int32))
            coins = (C.c_float * n)(*COINS[first:first + n])
            q4.check(L.q4_verify_sample_rows(s, buf.ptr + first * ld * 2, ld, n, coins, out.ptr))
            q4.synchronize()
            got = buf.get(np.uint16, 8 * ld).reshape(8, ld)
            tok = out.get(np.int32, 8)
            assert tok[:n].tolist() == toks[first:first + n], (first, tok.tolist(), toks)
            assert (tok[n:] == -9).all()
            assert (got[:, vocab:] == PAD).all(), "the padding behind a row was written"
            for r in range(8):
                if first <= r < first + n:
                    bad = np.flatnonzero(got[r, :vocab] != probs[r])
                    assert bad.size == 0, "row %d (launch of %d from %d): %d probabilities differ, first at %d" % (r, n, first, bad.size, bad[0])
                    top = got[r, :vocab].view(np.float16).astype(np.float32).max()
                    took.append(bool(top != 0 and top >= np.float32(COINS[r]) * np.float32(topp)))
                else:
                    assert np.array_equal(got[r, :vocab], rows[r].view(np.uint16)), "row %d is outside the launch and was written" % r
    finally:
        L.q4_sampler_delete(s)
    if 0 < topp < 1:         # from the kernel's own probabilities and coins: both branches of the search ran in this case
        assert any(took) and not all(took), took


@pytest.mark.parametrize("temperature,topp", [(1.0, 0.9), (0.8, 1.0)])
@pytest.mark.parametrize("vocab", [512, 16600, 32000])
def test_row_sampler_coin_1e_7(q4, orc, host, vocab, temperature, topp):
    """The coin 1e-7 itself, which the sampler's stream (multiples of 2^-24) cannot yield and the op-level entry can take: on the finite rows the token is
    the restatement's, and the probabilities -- which do not depend on the coin -- are q4_sample's."""
    L = q4.lib()
    rows = _rows(vocab)
    _, probs = _reference(q4, orc, host, vocab, temperature, topp)
    finite = [0, 1, 2, 3, 4, 5, 7]
    buf = q4.DevBuf(np.ascontiguousarray(rows[finite]))
    out = q4.DevBuf(np.full(8, -9, dtype=np.int32))
    coin = float(np.float32(1e-7))
    s = L.q4_sampler_new(vocab, temperature, topp, 1)
    try:
        q4.check(L.q4_verify_sample_rows(s, buf.ptr, vocab, 7, (C.c_float * 7)(*([coin] * 7)), out.ptr))
        q4.synchronize()
    finally:
        L.q4_sampler_delete(s)
    got = buf.get(np.uint16, 7 * vocab).reshape(7, vocab)
    tok = out.get(np.int32, 8)
    for i, r in enumerate(finite):
        assert np.array_equal(got[i], probs[r]), "row %d" % r
        assert tok[i] == orc.lib().orc_sample_topp(orc.f16_bits(rows[r].copy()), vocab, temperature, topp, coin), "row %d" % r
    assert tok[7] == -9


def test_row_sampler_refuses(q4, host):
    L = q4.lib()
    buf, out = q4.DevBuf(nbytes=8 * 40000 * 2), q4.DevBuf(nbytes=64)
    coins = (C.c_float * 8)()
    s = L.q4_sampler_new(512, 0.8, 0.9, 1)
    big = L.q4_sampler_new(40000, 0.8, 0.9, 1)
    odd = L.q4_sampler_new(516, 0.8, 0.9, 1)
    neg = L.q4_sampler_new(512, -0.7, 0.9, 1)
    zero = L.q4_sampler_new(512, 0.0, 0.9, 1)
    try:
        assert L.q4_verify_sample_rows(s, buf.ptr, 512, 0, coins, out.ptr) == 5 and L.q4_verify_sample_rows(s, buf.ptr, 512, 9, coins, out.ptr) == 5
        assert L.q4_verify_sample_rows(s, buf.ptr, 504, 2, coins, out.ptr) == 5 and L.q4_verify_sample_rows(s, buf.ptr, 516, 2, coins, out.ptr) == 5
        assert L.q4_verify_sample_rows(s, None, 512, 2, coins, out.ptr) == 5 and L.q4_verify_sample_rows(s, buf.ptr, 512, 2, None, out.ptr) == 5
        assert L.q4_verify_sample_rows(s, buf.ptr, 512, 2, coins, None) == 5
        for other, ld in ((big, 40000), (odd, 520), (neg, 512), (zero, 512)):
            assert L.q4_verify_sample_rows(other, buf.ptr, ld, 2, coins, out.ptr) == 1          # Q4_ERR_UNSUPPORTED_SIZE
    finally:
        for x in (s, big, odd, neg, zero):
            L.q4_sampler_delete(x)


# ---- 2. the accept launch on given tokens ------------------------------------------------------------------------------------------------------
def _accept_rows(size):
    r = np.random.default_rng(size)
    rows = (r.uniform(0, 1, (8, size))).astype(np.float16)
    rows[2, :] = 0
    rows[4, ::3] = np.nan
    return rows


@pytest.mark.parametrize("match", [0, 1, 3, 6, 7])
@pytest.mark.parametrize("size", [517, 1101])
def test_accept_tokens(q4, size, match):
    """the rows' tokens come from an array -- none of them a row's argmax, one the last id --: m, the ring, the position words, the report and the
    copies of row m against the restatement; everything else untouched"""
    rows = _accept_rows(size)
    ld = (size + 7) // 8 * 8
    D, p, dim = 7, 40, 64
    win = [5, size - 1, 9, 77, 300, 7, size - 3, 11]
    assert all(spec_ref.greedy_token(rows[i]) != win[i] for i in range(8))
    drafts = [win[i] if i < match else _wrong(win[i]) for i in range(D)]
    m = ref.accept_tokens(win, drafts)
    assert m == match
    padded = np.zeros((8, ld), dtype=np.float16)
    padded[:, :size] = rows
    padded[:, size:] = 60000.0
    x = np.random.default_rng(3).standard_normal((8, dim)).astype(np.float16)
    dl, dx, dw = q4.DevBuf(padded), q4.DevBuf(x), q4.DevBuf(np.array(win, dtype=np.int32))
    lo, xo = q4.DevBuf(nbytes=ld * 2), q4.DevBuf(nbytes=dim * 2)
    ring = q4.DevBuf(np.full(64, -7, dtype=np.int32))
    ph, pd = q4.DevBuf(np.array([p], dtype=np.int32)), q4.DevBuf(np.array([p], dtype=np.int32))
    rep = q4.DevBuf(np.full(9, -3, dtype=np.int32))
    q4.verify_accept_tokens(dl, ld, size, drafts, dw, dx, dim, lo, xo, ring, ph, pd, rep)
    q4.synchronize()
    assert rep.get(np.int32, 9).tolist() == win + [m]
    got_ring = ring.get(np.int32, 64)
    assert got_ring[p + 1:p + m + 2].tolist() == win[:m + 1]
    assert (got_ring[:p + 1] == -7).all() and (got_ring[p + m + 2:] == -7).all()
    assert ph.get(np.int32, 1)[0] == p + m + 1 and pd.get(np.int32, 1)[0] == p + m + 1
    assert np.array_equal(lo.get(np.uint16, size), rows[m].view(np.uint16))
    assert not lo.get(np.uint16, ld)[size:].any()
    assert np.array_equal(xo.get(np.uint16, dim), x[m].view(np.uint16))
    assert np.array_equal(dl.get(np.uint16, 8 * ld), padded.view(np.uint16).ravel(), equal_nan=False)
    assert dw.get(np.int32, 8).tolist() == win and np.array_equal(dx.get(np.uint16, 8 * dim), x.view(np.uint16).ravel())
    # fewer drafts than rows: the report ends at row n_draft
    rep2 = q4.DevBuf(np.full(9, -3, dtype=np.int32))
    q4.verify_accept_tokens(dl, ld, size, drafts[:3], dw, dx, dim, lo, xo, ring, ph, pd, rep2)
    q4.synchronize()
    assert rep2.get(np.int32, 9).tolist() == win[:4] + [-1] * 4 + [min(m, 3)]


def test_accept_tokens_refuses_bad_arguments(q4):
    L = q4.lib()
    b = q4.DevBuf(nbytes=4096)
    d = (C.c_int * 8)(*range(8))
    args = lambda ld, size, nd, win=b.ptr: (b.ptr, ld, size, d, nd, win, None, 64, b.ptr, None, b.ptr, b.ptr, b.ptr, None)
    assert L.q4_verify_accept_tokens(*args(520, 517, 0)) == 5 and L.q4_verify_accept_tokens(*args(520, 517, 8)) == 5
    assert L.q4_verify_accept_tokens(*args(517, 517, 3)) == 5 and L.q4_verify_accept_tokens(*args(512, 517, 3)) == 5
    assert L.q4_verify_accept_tokens(*args(520, 517, 3, None)) == 5


# ---- 3. the primitive --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def stepwise(q4, models):
    """R: the per-token sampled run (T 0.8, p 0.9, seed 7) of the 17-token prompt to 150 steps through the per-step entry point, with what every step
    leaves in RunState::logits (a generating step: the fp16 probabilities)"""
    q4.lib().q4_set_use_graphs(1)
    t = q4.Transformer(models["ffn_pair7b"], temperature=TEMP, topp=TOPP, seed=RNG)
    t.reset(_prompt())
    logits = []
    for pos in range(STEPS):
        t.run_transformer_at(pos, pos >= N_PROMPT - 1)
        logits.append(t.logits().view(np.uint16).copy())
    q4.synchronize()
    ring = np.array([t.token(i) for i in range(STEPS + 1)], dtype=np.int32)
    kv, _ = _state(t, STEPS)
    assert _rng_state(t) == ref.draw(RNG, STEPS)[1]
    assert not t.speculative_sampled() and t.speculative() == {"draft": 0, "ngram": 0, "min": 0} and t.spec_stats() == (0, 0, 0)     # off unless asked for
    t.set_speculative(draft=0, sampled=True)
    assert t.speculative_sampled() and t.speculative() == {"draft": 0, "ngram": 0, "min": 0}
    yield {"t": t, "ring": ring, "logits": logits, "kv": kv}
    t.close()


@pytest.mark.parametrize("D", [1, 3, 7])
@pytest.mark.parametrize("p", [16, 60, 123, 126])
def test_primitive(q4, stepwise, p, D):
    """q4_verify_tokens_sampled at position p with D drafts whose first wrong index k takes every value 0 .. D: n_accepted, the emitted tokens, the
    position, the probabilities there and the Sampler's state after p + k + 1 draws; then per-token steps to 150 over the rows the pass left."""
    t, R = stepwise["t"], stepwise["ring"]
    for k in range(D + 1):
        ref.sampler_struct(t.sampler).rng_state = RNG
        t.generate_ids(R[:N_PROMPT], p)                               # per-token (and prompt passes) to position p: ring[p] is R's
        assert t.pos() == p and _rng_state(t) == ref.draw(RNG, p)[1]  # the stream stands at position p's coin
        assert t.verify_covers_sampled(p, D)
        drafts = [int(R[p + 1 + i]) for i in range(D)]
        if k < D:
            drafts[k] = _wrong(R[p + 1 + k])
        before = t.spec_stats()
        emitted, acc = t.verify_sampled(drafts)
        assert acc == k, "p %d, D %d, first wrong %d: accepted %d" % (p, D, k, acc)
        assert emitted.tolist() == R[p + 1:p + k + 2].tolist()
        assert t.pos() == p + k + 1
        assert np.array_equal(t.logits().view(np.uint16), stepwise["logits"][p + k]), "probabilities behind the pass (p %d, D %d, k %d)" % (p, D, k)
        assert _rng_state(t) == ref.draw(RNG, p + k + 1)[1], "the Sampler's state behind the pass (p %d, D %d, k %d)" % (p, D, k)
        after = t.spec_stats()
        assert (after[0] - before[0], after[1] - before[1], after[2] - before[2]) == (1, D, k)
        ref.sampler_struct(t.sampler).rng_state = RNG                 # (the loop draws and discards the skipped steps' coins)
        toks = t.generate_ids_from(R[:p + k + 2], STEPS, p + k + 1)[0]
        assert np.array_equal(toks, R), "ring behind the pass (p %d, D %d, k %d)" % (p, D, k)
        kv, logits = _state(t, STEPS)
        bad = np.unique(np.argwhere(kv != stepwise["kv"])[:, 0])
        assert bad.size == 0, "K / V rows differ at positions %s (p %d, D %d, k %d)" % (bad[:8], p, D, k)
        assert np.array_equal(logits, stepwise["logits"][STEPS - 1])
        assert _rng_state(t) == ref.draw(RNG, STEPS)[1]


def test_primitive_arguments_and_admission(q4, stepwise, models):
    t, R = stepwise["t"], stepwise["ring"]
    L = q4.lib()
    ref.sampler_struct(t.sampler).rng_state = RNG
    t.generate_ids(R[:N_PROMPT], 30)
    rng = _rng_state(t)
    out, acc = (C.c_int * 9)(), C.c_int()
    ids = lambda *a: (C.c_int * len(a))(*a)
    for bad, n in ((ids(512), 1), (ids(-1), 1), (ids(5, 600), 2), (ids(*range(8)), 8), (ids(5), 0)):
        assert L.q4_verify_tokens_sampled(t.h, t.sampler, bad, n, out, C.byref(acc)) == 5
    assert L.q4_verify_tokens_sampled(t.h, t.sampler, None, 1, out, C.byref(acc)) == 5
    assert L.q4_verify_tokens_sampled(t.h, None, ids(5), 1, out, C.byref(acc)) == 5
    assert t.pos() == 30 and _rng_state(t) == rng
    assert t.verify_covers_sampled(248, 7) and not t.verify_covers_sampled(249, 7) and t.verify_covers_sampled(254, 1) and not t.verify_covers_sampled(255, 1)
    # the switch off: not admitted, nothing runs, the position and the stream stay
    t.set_speculative(draft=0, sampled=False)
    before = t.spec_stats()
    assert not t.verify_covers_sampled(30, 1) and t.verify_sampled([int(R[31])]) is None
    assert t.pos() == 30 and t.spec_stats() == before and _rng_state(t) == rng
    t.set_speculative(draft=0, sampled=True)
    assert t.verify_sampled([int(R[31])])[1] == 1 and _rng_state(t) == ref.draw(RNG, 32)[1]


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
@pytest.mark.parametrize("temperature,topp", [(0.8, 0.9), (0.7, 1.0)])
@pytest.mark.parametrize("kind", ["oracle", "wrong", "alternating"])
@pytest.mark.parametrize("name", ["ffn_pair7b", "ffn_pair_ragged", "spec_cls_ragged"])
def test_loop_forced_drafters(q4, models, name, kind, temperature, topp, graphs):
    off = _off(q4, models, name, graphs, temperature=temperature, topp=topp)
    R = off["tokens"]
    on = _run(q4, models[name], graphs, spec=SPEC, drafter=DRAFTERS[kind](R), temperature=temperature, topp=topp, seed=RNG)
    _assert_same(off, on, "%s, %s drafter, T %g, p %g, graphs %d" % (name, kind, temperature, topp, graphs))
    want, passes = spec_ref.replay(R, N_PROMPT, STEPS, DRAFTERS[kind](R), 7, lambda pos: off["groups"][pos] if graphs == 1 else 1)
    assert on["stats"] == want, (on["stats"], want)
    assert want[0] >= 10
    if kind == "oracle":
        assert want[1] == want[2] and all(p[1] == 7 for p in passes[:-1])       # every pass accepts everything; only the last may be cut by `steps`
    if kind == "wrong":
        assert want[2] == 0


# ---- 5. the loop with the built-in drafter under sampling --------------------------------------------------------------------------------------
BUILTIN = dict(temperature=0.03, topp=0.9, seed=7)


def test_loop_builtin_drafter(q4, models):
    """n-grams 3 .. 1, 7 drafts, 250 steps at a temperature low enough that the run repeats itself. The off run must itself contain at least three
    passes with an accepted draft and one with none. Chosen with the CPU oracle (oracle.Model.forward + orc_sample_topp over the same coin stream and
    spec_ref.replay with groups of 8): T 0.03, p 0.9, seed 7 gives 8 passes, 55 drafts, 5 accepted -- 4 passes with an accepted draft, 4 with none;
    (0.02, 0.9, 3) gave 3 / 10, (0.08, 0.6, 5) 3 / 11, (0.05, 0.9, 7) 1 / 8, (0.1, 0.9, 7) 1 / 11, (0.5, 0.6, 7) 0 / 4. The GPU's tokens may drift from
    the oracle's, so the condition is asserted on the GPU's own off run."""
    steps = 250
    off = _off(q4, models, "ffn_pair7b", 1, steps, **BUILTIN)
    R = off["tokens"]
    builtin = lambda ring, room: spec_ref.draft(ring, room, 3, 1)
    want, passes = spec_ref.replay(R, N_PROMPT, steps, builtin, 7, lambda pos: off["groups"][pos])
    print("built-in drafter over the sampled off run: passes, drafted, accepted = %s; distinct tokens %d" % (want, len(set(R.tolist()))))
    assert sum(1 for p in passes if p[2] > 0) >= 3 and sum(1 for p in passes if p[2] == 0) >= 1, passes
    on = _run(q4, models["ffn_pair7b"], 1, steps=steps, spec=SPEC, **BUILTIN)
    _assert_same(off, on, "built-in drafter")
    assert on["stats"] == want, (on["stats"], want)


# ---- 6. not admitted ---------------------------------------------------------------------------------------------------------------------------
def _guide(q4):
    return q4.Guide(np.zeros((1, 512), dtype=np.uint16))               # one state that allows every token


@pytest.mark.parametrize("case", ["switch_off", "top_k", "dry", "adaptive", "guide", "logprobs", "fp8", "fusion1", "tiny", "negative"])
def test_not_admitted_runs_the_steps(q4, models, case):
    L = q4.lib()
    name, kw, level, steps, spec = "ffn_pair7b", dict(temperature=TEMP, topp=TOPP, seed=RNG), None, 60, SPEC
    if case == "switch_off":
        spec = dict(draft=7, ngram=3, min=1)
    elif case == "top_k":
        kw["sampling"] = dict(top_k=5)
    elif case == "dry":
        kw["dry"] = dict(multiplier=0.8)
    elif case == "adaptive":
        kw["adaptive"] = dict(typical_p=0.9)
    elif case == "guide":
        kw["guide"] = _guide(q4)
    elif case == "logprobs":
        kw["logprobs"] = 0
    elif case == "fp8":
        kw["kv"] = "fp8"
    elif case == "fusion1":
        level = 1
    elif case == "tiny":
        name, steps = "tiny", 40
    elif case == "negative":
        kw["temperature"] = -0.7
    calls = []

    def drafter(ring, room):
        calls.append(len(ring))
        return [5] * room
    try:
        if level is not None:
            L.q4_set_fusion(level)
        off = _run(q4, models[name], 1, steps=steps, **kw)
        on = _run(q4, models[name], 1, steps=steps, spec=spec, drafter=drafter, **kw)
    finally:
        if level is not None:
            L.q4_set_fusion(q4.DEFAULT_FUSION)
        if "guide" in kw:
            kw["guide"].close()
    assert on["stats"] == (0, 0, 0) and calls == []
    _assert_same(off, on, case)


def test_vocabulary_above_the_on_chip_form_is_not_covered(q4, models):
    for name, temperature, covered in (("v40k", TEMP, False), ("ffn_pair7b", TEMP, True), ("ffn_pair7b", -0.7, False), ("ffn_pair7b", 0.0, False),
                                       ("ffn_pair7b", float("inf"), False)):
        t = q4.Transformer(models[name], temperature=temperature, topp=TOPP, seed=RNG)
        try:
            t.set_speculative(draft=7, sampled=True)
            assert t.verify_covers_sampled(20, 3) == covered, (name, temperature)
        finally:
            t.close()


def test_the_switch_leaves_greedy_verification_alone(q4, models):
    greedy = _run(q4, models["ffn_pair7b"], 1, groups=True)
    R = greedy["tokens"]
    a = _run(q4, models["ffn_pair7b"], 1, spec=dict(draft=7, ngram=3, min=1, sampled=False), drafter=_alternating(R))
    b = _run(q4, models["ffn_pair7b"], 1, spec=SPEC, drafter=_alternating(R))
    _assert_same(greedy, a, "greedy, sampled off")
    _assert_same(a, b, "greedy, sampled on")
    assert a["stats"] == b["stats"] and a["stats"][0] >= 10 and 0 < a["stats"][2] < a["stats"][1]


# ---- 7. afterwards -----------------------------------------------------------------------------------------------------------------------------
def test_second_generation_equals_a_fresh_one(q4, models):
    off = _off(q4, models)
    R = off["tokens"]
    second = _prompt(N_PROMPT + 3, seed=21)
    fresh = _run(q4, models["ffn_pair7b"], 1, prompt=second, steps=60, temperature=TEMP, topp=TOPP, seed=RNG)
    L = q4.lib()
    t = q4.Transformer(models["ffn_pair7b"], speculative=SPEC, temperature=TEMP, topp=TOPP, seed=RNG)
    try:
        assert t.speculative() == {"draft": 7, "ngram": 3, "min": 1} and t.speculative_sampled()
        t.set_drafter(_alternating(R))
        assert np.array_equal(t.generate_ids(_prompt(), STEPS)[0], R)
        assert t.spec_stats()[0] > 0 and _rng_state(t) == off["rng"]
        t.set_drafter(None)
        t.set_speculative(draft=0)
        assert not t.speculative_sampled()
        ref.sampler_struct(t.sampler).rng_state = RNG
        again = {"tokens": t.generate_ids(second, 60)[0].copy(), "rng": _rng_state(t)}
        q4.check(L.q4_handoff_status(t.state))
        again["kv"], again["logits"] = _state(t, 60)
    finally:
        t.close()
    _assert_same(fresh, again, "second generation")


def test_common_prefix_behind_rejected_drafts(q4, models):
    """A sampled pass whose drafts are all rejected leaves draft rows above the position: the common prefix stops at the position, and a generation
    that reuses it gives the full run's bytes"""
    off = _off(q4, models)
    R = off["tokens"]
    t = q4.Transformer(models["ffn_pair7b"], temperature=TEMP, topp=TOPP, seed=RNG)
    try:
        t.set_speculative(draft=0, sampled=True)
        t.generate_ids(R[:N_PROMPT], 60)
        emitted, acc = t.verify_sampled([_wrong(R[61])] + [int(x) for x in R[62:68]])
        assert acc == 0 and emitted.tolist() == [int(R[61])] and t.pos() == 61 and _rng_state(t) == ref.draw(RNG, 61)[1]
        assert t.common_prefix(R[:100]) == 61
        ref.sampler_struct(t.sampler).rng_state = RNG
        toks = t.generate_ids(R[:62], STEPS, reuse=True)
        assert toks[2] == STEPS - 1 - 61                             # the steps that ran
        got = {"tokens": toks[0].copy(), "rng": _rng_state(t)}
        got["kv"], got["logits"] = _state(t, STEPS)
    finally:
        t.close()
    _assert_same(off, got, "reused prefix behind a sampled pass")


def test_snapshot_after_a_sampled_speculative_run(q4, models):
    off = _off(q4, models)
    R = off["tokens"]
    t = q4.Transformer(models["ffn_pair7b"], speculative=SPEC, temperature=TEMP, topp=TOPP, seed=RNG)
    t2 = None
    try:
        t.set_drafter(_alternating(R))
        first = t.generate_ids(_prompt(), 100)[0]
        assert np.array_equal(first, R[:101]) and t.spec_stats()[0] > 0
        snap = t.snapshot()
        assert snap.n_pos == 100
        t2 = q4.Transformer(models["ffn_pair7b"], temperature=TEMP, topp=TOPP, seed=RNG)
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


def test_beyond_position_256(q4, tmp_path_factory):
    """q4_set_pass_context raised: sampled passes follow the steps into the split-context bins (pass_long; the run crosses position 256)"""
    path = str(tmp_path_factory.mktemp("speculative_sampled_long") / "pass_long.bin")
    synth.write_model(path, "pass_long", seed=SEED)
    steps = 300
    kw = dict(temperature=TEMP, topp=TOPP, seed=RNG)
    q4.set_pass_context(2304)
    try:
        off = _run(q4, path, 1, steps=steps, groups=True, **kw)
        R = off["tokens"]
        assert 2 not in R[1:].tolist()
        seen = []

        def drafter(ring, room):
            seen.append((len(ring) - 1, room))
            return R[len(ring):len(ring) + room]
        on = _run(q4, path, 1, steps=steps, spec=SPEC, drafter=drafter, **kw)
    finally:
        q4.set_pass_context(256)
    _assert_same(off, on, "300 positions, pass context 2304")
    assert on["stats"][0] >= 20 and on["stats"][1] == on["stats"][2]
    assert any(pos >= 256 for pos, _ in seen) and all(pos + room < 256 or pos >= 256 for pos, room in seen)      # no pass reaches across the bin's end
