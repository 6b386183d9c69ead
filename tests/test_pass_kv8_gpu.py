"""Prompt and verify passes on the FP8 (e4m3) K / V cache (q4_set_pass_kv8; csrc/prompt_pass_kv8.hip, DESIGN.md 3.7 "FP8 cache"). A pass leaves its K / V
rows in fp16 staging rows, one launch per layer quantises and appends them as the step's attention launch appends its row, and attention then reads
every row from the byte caches -- the bytes the step holds in registers for its current row. So "equal" always means BYTE-equal against the same library
running per-token steps (prompt ingest off, the switch off) on a fresh Transformer(path, kv="fp8"): the token ring, the position, the final logits, the
sampler's rng_state, q4_get_kv_row of every layer and position below the final one, and the raw e4m3 bytes and row exponents through the
q4_snapshot_export blob of that prefix. No tolerance anywhere.

Models: `pass_long` (7B width, 2 layers, context 2304, vocabulary 512) and, for the grouped-query composition, `gqa7b_pair`."""
import ctypes as C
import hashlib

import numpy as np
import pytest

import hostile_models as hm
import pass_context_ref as ref
import test_speculative_gpu as tsg
from llama_cu_awq_amd import synth
from test_pass_logprobs_gpu import _records, _score
from test_prompt_ingest_gpu import _expected_passes

pytestmark = pytest.mark.gpu

NAME = "pass_long"
GQA = "gqa7b_pair"
SEED = 11
T = 8                     # PROMPT_PASS_MAX
GEN = 6
S = 2304                  # both models' context, and the bound the long tests raise the setting to
N_LONG = 2200
CACHES = ("key_cache", "value_cache")
POISON = ("nan", "max")   # every byte 0x7F (an e4m3fn NaN); 0x7E / 0xFE alternating (+448 / -448)


@pytest.fixture(scope="module")
def models(tmp_path_factory):
    d = tmp_path_factory.mktemp("pass_kv8")
    made = {}

    def get(name=NAME, trait=None):
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
_REPEAT = [1] + [int(x) for x in np.random.default_rng(3).integers(3, 512, size=9)] * 5


def _wrong(tok):
    w = (int(tok) + 1) % 512
    return w + 1 if w == 2 else w


# ---- where an FP8 pass is admitted: csrc/q4_passes.hip pass_attention_plan's FP8 branch, restated on positions ------------------------------------------
def _form(pos, mode):
    """'o' (the one-pass form, bin argument <= 256), the chunk of the split-context form (128 up to argument 1024, 256 above), or None: a one-pass step
    above 256 (no graphs: arguments 257 .. 511), which has no row form"""
    arg = ref.bin_arg(pos, mode, S)
    if arg >= ref.SPLIT_MIN:
        return 128 if arg <= 1024 else 256
    return "o" if arg <= 256 else None


def _covers(pos, n, bound, mode):
    if n < 1 or pos + n > min(max(bound, 256), S) or pos + n > ref.bin_end(pos):
        return False
    kinds = {_form(pos + i, mode) for i in range(n)}
    return None not in kinds and len(kinds) == 1


def _passes(n_prompt, steps, bound, start=0, mode=1, ingest=T):
    """tests/pass_context_ref.py's prompt_passes with the FP8 forms"""
    out, pos, last = [], start, min(n_prompt - 1, steps)
    while pos < last:
        n = min(last - pos, ingest, ref.bin_end(pos) - pos, min(max(bound, 256), S) - pos)
        if n >= 2 and _covers(pos, n, bound, mode):
            out.append((pos, n))
            pos += n
        else:
            pos += 1
    return out


def test_plan_restated():
    """the restatement itself: below 256 it is _expected_passes; without graphs position 511 is split while 510 is one-pass above 256, so no pass touches
    256 .. 511 there; with graphs [256, 512) is one split stretch"""
    for n in (3, 9, 130, 250, 257):
        assert len(_passes(n, n + GEN, S)) == _expected_passes(n)
    assert _form(510, 0) is None and _form(511, 0) == 128 and _form(1023, 0) == 128 and _form(1024, 0) == 256
    assert all(pos + n <= 256 or pos >= 512 for pos, n in _passes(700, 706, S, mode=0))
    assert _form(256, 1) == 128 and _form(511, 1) == 128 and _form(1024, 1) == 256


# ---- the byte caches, raw ------------------------------------------------------------------------------------------------------------------------------
def _shape(t):
    cfg = t.config
    return cfg.n_layers, cfg.seq_len, cfg.dim * cfg.n_kv_heads // cfg.n_heads


def _poison_row(pattern, kv_dim):
    if pattern == "nan":
        return np.full(kv_dim, 0x7F, dtype=np.uint8)
    assert pattern == "max", pattern
    return np.where(np.arange(kv_dim) % 2 == 0, 0x7E, 0xFE).astype(np.uint8)


def _address(t, cache, layer, row):
    _, seq_len, kv_dim = _shape(t)
    return getattr(t.state.contents, cache) + (layer * seq_len + row) * kv_dim       # one byte per element


def _poison(q4, t, first_row, pattern):
    """rows [first_row, seq_len) of every layer of both byte caches become the pattern"""
    L = q4.lib()
    n_layers, seq_len, kv_dim = _shape(t)
    assert 0 <= first_row < seq_len and t.kv_format == "fp8"
    block = np.ascontiguousarray(np.tile(_poison_row(pattern, kv_dim), (seq_len - first_row, 1)))
    q4.check(L.q4_stream_synchronize())
    for cache in CACHES:
        for layer in range(n_layers):
            q4.check(L.q4_memcpy_h2d(_address(t, cache, layer, first_row), block.ctypes.data, block.nbytes))
    q4.check(L.q4_stream_synchronize())


def _assert_untouched(q4, t, first_row, pattern, what):
    L = q4.lib()
    n_layers, seq_len, kv_dim = _shape(t)
    want = _poison_row(pattern, kv_dim)
    q4.check(L.q4_stream_synchronize())
    for cache in CACHES:
        for layer in range(n_layers):
            got = np.empty((seq_len - first_row, kv_dim), dtype=np.uint8)
            q4.check(L.q4_memcpy_d2h(got.ctypes.data, _address(t, cache, layer, first_row), got.nbytes))
            bad = np.flatnonzero((got != want).any(axis=1))
            assert bad.size == 0, "%s: %s rows of layer %d written above row %d: %s" % (what, cache, layer, first_row, (bad[:8] + first_row).tolist())


def _rows(t, first, n):
    """q4_get_kv_row of every layer for positions [first, first + n): uint16 [n, layers * 2 * kv_dim]"""
    if n <= 0:
        return np.empty((0, 0), dtype=np.uint16)
    return np.stack([np.concatenate([np.concatenate(t.kv_row(l, pos)) for l in range(t.config.n_layers)]) for pos in range(first, first + n)]).view(np.uint16).copy()


def _blob(t, n_pos):
    """the q4_snapshot_export blob of positions [0, n_pos) -- the e4m3 bytes and both exponent arrays of every layer -- as a digest"""
    snap = t.snapshot(n_pos)
    try:
        b = snap.to_bytes()
        assert snap.info["kv_format"] == 1 and len(b) > n_pos * 2 * _shape(t)[0] * _shape(t)[2]
        return hashlib.sha256(b).hexdigest()
    finally:
        snap.close()


def _capture(q4, t, toks=None):
    q4.check(q4.lib().q4_handoff_status(t.state))
    pos = t.pos()
    if toks is None:
        toks = np.array([t.token(i) for i in range(pos + 1)], dtype=np.int32)
    return dict(tokens=np.asarray(toks).copy(), pos=pos, logits=t.logits().view(np.uint16).copy(), rng=tsg._rng_state(t), rows=_rows(t, 0, pos),
                blob=_blob(t, pos), stats=t.spec_stats())


def _run(q4, path, prompt, steps=None, kv8=True, ingest=T, graphs=1, bound=256, start=0, warm=None, poison=None, spec=None, drafter=None, reuse=None, **kw):
    """One generation on a fresh Transformer(kv="fp8"): _capture plus passes. warm: a prompt generated first (start > 0 reuses its prefix). poison:
    (pattern, first row) written behind the warm run; the rows from T above the final position must then still hold it. reuse: a Snapshot restored first."""
    L = q4.lib()
    default = L.q4_get_prompt_ingest()
    timeouts = L.q4_handoff_timeouts()
    try:
        L.q4_set_use_graphs(graphs)
        L.q4_set_prompt_ingest(ingest)
        q4.set_pass_context(bound)
        t = q4.Transformer(path, kv="fp8", pass_kv8=kv8, **kw)
        try:
            assert t.pass_kv8() == bool(kv8) and t.kv_format == "fp8"
            if warm is not None:
                t.generate_ids(warm, len(warm) + GEN)
            if poison is not None:
                _poison(q4, t, poison[1], poison[0])
            if spec is not None:
                t.set_speculative(**spec)
            if drafter is not None:
                t.set_drafter(drafter)
            steps = len(prompt) + GEN if steps is None else steps
            before = L.q4_prompt_passes()
            if reuse is not None:
                toks = t.generate_ids(prompt, steps, reuse=reuse)[0].copy()
            else:
                toks = t.generate_ids_from(prompt, steps, start)[0].copy()
            passes = L.q4_prompt_passes() - before
            out = _capture(q4, t, toks)
            out["passes"] = passes
            assert L.q4_handoff_timeouts() == timeouts
            if poison is not None and out["pos"] + T < t.config.seq_len:
                _assert_untouched(q4, t, out["pos"] + T, poison[0], "final position %d" % out["pos"])
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
    assert a["rows"].shape == b["rows"].shape
    bad = np.flatnonzero((a["rows"] != b["rows"]).any(axis=1))
    assert bad.size == 0, "%s: K / V rows (q4_get_kv_row) differ at positions %s" % (what, bad[:8].tolist())
    assert a["blob"] == b["blob"], "%s: the snapshot blobs (e4m3 bytes, row exponents) differ" % what
    assert np.array_equal(a["logits"], b["logits"]), "%s: final logits differ in %d entries" % (what, int((a["logits"] != b["logits"]).sum()))
    assert not rng or a["rng"] == b["rng"], "%s: the Sampler's random state differs" % what


_OFF = {}


def _off(q4, models, n_prompt, graphs=1, name=NAME, trait=None):
    """the per-token run (prompt ingest off, the switch off), computed once per case and shared"""
    key = (name, trait, n_prompt, graphs)
    if key not in _OFF:
        _OFF[key] = _run(q4, models(name, trait), _LONG[:n_prompt], kv8=False, ingest=0, graphs=graphs)
        assert _OFF[key]["passes"] == 0
    return _OFF[key]


# ---- 1. prompt passes --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graphs", [1, 0])
@pytest.mark.parametrize("ingest", [8, 5, 3])
@pytest.mark.parametrize("n_prompt", [3, 9, 130, 250, 257, 300, 700, 1100, 2200])
def test_prompt_passes(q4, models, n_prompt, ingest, graphs):
    """passes of 8, 5 and 3 straddle the 128- and 256-position chunk boundaries and stop at every stretch end; without graphs positions 256 .. 511 run
    steps (one-pass above 256, and 511 split alone)"""
    off = _off(q4, models, n_prompt, graphs)
    on = _run(q4, models(), _LONG[:n_prompt], ingest=ingest, graphs=graphs, bound=S if n_prompt > 256 else 256)
    want = len(_passes(n_prompt, n_prompt + GEN, S, mode=graphs, ingest=ingest))
    print("%d prompt tokens, passes of %d, graphs %d: %d passes (expected %d)" % (n_prompt, ingest, graphs, on["passes"], want))
    assert on["passes"] == want
    if ingest == T and n_prompt <= 257:
        assert want == _expected_passes(n_prompt)
    assert want > 0 or n_prompt == 3 and ingest == 3
    _assert_same(off, on, "%d prompt tokens, passes of %d, graphs %d" % (n_prompt, ingest, graphs))


@pytest.mark.parametrize("graphs", [1, 0])
@pytest.mark.parametrize("n_prompt", [9, 250, 700])
def test_switch_off_runs_no_pass(q4, models, n_prompt, graphs):
    """the switch off, ingest on, the bound raised: an FP8 model runs no pass, the probe says 0, the bytes are the steps'"""
    off = _off(q4, models, n_prompt, graphs)
    plain = _run(q4, models(), _LONG[:n_prompt], kv8=False, graphs=graphs, bound=S)
    assert plain["passes"] == 0
    _assert_same(off, plain, "switch off, %d prompt tokens" % n_prompt)


def test_switch_and_probe(q4, models):
    q4.set_pass_context(S)
    t = q4.Transformer(models(), kv="fp8")
    try:
        assert not t.pass_kv8() and not any(t.verify_covers(p, 4) for p in (0, 30, 300, 640, 1100, 2100))
        t.set_pass_kv8(True)
        assert t.pass_kv8() and all(t.verify_covers(p, 4) for p in (0, 30, 300, 640, 1100, 2100))
        assert t.verify_covers(248, 7) and not t.verify_covers(249, 7) and not t.verify_covers(508, 4) and t.verify_covers(507, 4)
        t.set_pass_kv8(False)
        assert not t.pass_kv8() and not t.verify_covers(30, 4)
    finally:
        q4.set_pass_context(256)
        t.close()


def test_fp16_model_is_unchanged(q4, models):
    """a model with the fp16 cache and the switch on: the pass counts and bytes it has with the switch off"""
    res = {}
    for on in (False, True):
        t = q4.Transformer(models(), pass_kv8=on)
        try:
            before = q4.prompt_passes()
            toks = t.generate_ids(_LONG[:140], 146)[0].copy()
            res[on] = (q4.prompt_passes() - before, toks, t.logits().view(np.uint16).copy(), _rows(t, 0, t.pos()))
        finally:
            t.close()
    assert res[False][0] == res[True][0] == _expected_passes(140)
    assert all(np.array_equal(a, b) for a, b in zip(res[False][1:], res[True][1:]))


# ---- 2. verify passes ----------------------------------------------------------------------------------------------------------------------------------------
_STEPWISE = {}


def _stepwise(q4, path, p, D=7, **kw):
    """P[:p + 1] stepped to position p, then D + 1 generating steps one by one: the true continuation R[p + 1 .. p + D + 1] and, behind step i, the logits,
    the rng_state and the blob of the prefix [0, p + i + 1); the rows [p, p + D + 1) at the end"""
    key = (path, p, D, tuple(sorted(kw.items())))
    if key in _STEPWISE:
        return _STEPWISE[key]
    L = q4.lib()
    L.q4_set_prompt_ingest(0)
    t = q4.Transformer(path, kv="fp8", **kw)
    try:
        t.generate_ids(_LONG[:p + 1], p)
        assert t.pos() == p
        logits, rng, blobs = [], [], []
        for i in range(D + 1):
            t.run_transformer(True)
            q4.synchronize()
            assert t.pos() == p + i + 1
            logits.append(t.logits().view(np.uint16).copy())
            rng.append(tsg._rng_state(t))
            blobs.append(_blob(t, p + i + 1))
        q4.check(L.q4_handoff_status(t.state))
        _STEPWISE[key] = {"R": [t.token(i) for i in range(p + D + 2)], "logits": logits, "rng": rng, "blobs": blobs, "rows": _rows(t, p, D + 1)}
        return _STEPWISE[key]
    finally:
        t.close()
        L.q4_set_prompt_ingest(T)


def _verify_all_indices(q4, path, p, D, poison=None, **kw):
    """q4_verify_tokens at position p with D drafts, the true continuation wrong at index k for every k in 0 .. D (k = D: all right), each on rows
    ingested afresh by passes over whatever the case in front left above the position"""
    L = q4.lib()
    want = _stepwise(q4, path, p, **kw)
    R = want["R"]
    q4.set_pass_context(S)
    t = q4.Transformer(path, kv="fp8", pass_kv8=True, **kw)
    try:
        for k in range(D + 1):
            before = L.q4_prompt_passes()
            t.generate_ids(_LONG[:p + 1], p)
            assert t.pos() == p and L.q4_prompt_passes() - before == len(_passes(p + 1, p, S))
            assert t.verify_covers(p, D)
            if poison is not None:
                _poison(q4, t, p, poison)
            drafts = [int(x) for x in R[p + 1:p + 1 + D]]
            if k < D:
                drafts[k] = _wrong(drafts[k])
            stats = t.spec_stats()
            emitted, acc = t.verify(drafts)
            what = "position %d, %d drafts, first wrong %d" % (p, D, k)
            assert acc == k and emitted.tolist() == R[p + 1:p + k + 2], what
            assert t.pos() == p + k + 1 and [t.token(i) for i in range(p + k + 2)] == R[:p + k + 2], what
            assert t.spec_stats() == (stats[0] + 1, stats[1] + D, stats[2] + k), what
            assert np.array_equal(t.logits().view(np.uint16), want["logits"][k]), what + ": logits behind the pass"
            got = _rows(t, p, k + 1)
            bad = np.flatnonzero((got != want["rows"][:k + 1]).any(axis=1))
            assert bad.size == 0, "%s: K / V rows differ at positions %s" % (what, (bad + p).tolist())
            assert _blob(t, p + k + 1) == want["blobs"][k], what + ": the snapshot blobs (e4m3 bytes, row exponents) differ"
            if poison is not None:
                _assert_untouched(q4, t, p + D + 1, poison, what)
            q4.check(L.q4_handoff_status(t.state))
    finally:
        q4.set_pass_context(256)
        t.close()


@pytest.mark.parametrize("D", [1, 4, 7])
@pytest.mark.parametrize("p", [30, 200, 300, 640, 1100, 2100])
def test_verify_tokens(q4, models, p, D):
    _verify_all_indices(q4, models(), p, D)


def test_speculative_loop(q4, models):
    """the token loop with the built-in n-gram drafter on a repeating prompt: the run without speculation byte for byte, and drafts were accepted"""
    kw = dict(steps=len(_REPEAT) + 150)
    off = _run(q4, models(), _REPEAT, kv8=False, ingest=0, **kw)
    on = _run(q4, models(), _REPEAT, spec=dict(draft=4, ngram=3, min=1), **kw)
    print("passes, drafted, accepted = %s" % (on["stats"],))
    assert off["stats"] == (0, 0, 0) and on["passes"] == _expected_passes(len(_REPEAT))
    assert on["stats"][0] > 0 and on["stats"][2] > 0, on["stats"]
    _assert_same(off, on, "speculative loop")


# ---- 3. resume -------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("start,n", [(5, 140), (300, 700)])
def test_resumed(q4, models, start, n):
    """generate_ids_from over a warm prefix (itself ingested by passes), the start no multiple of 8: the full per-token run's bytes"""
    prompt = _LONG[:n]
    off = _off(q4, models, n)
    on = _run(q4, models(), prompt, bound=S, start=start, warm=prompt[:start] + _prompt(40, seed=9)[1:])
    assert on["passes"] == len(_passes(n, n + GEN, S, start=start)) > 0
    _assert_same(off, on, "resumed at %d" % start, rng=False)         # (the warm generation may have drawn coins of its own)


def test_restored_snapshot(q4, models):
    """a snapshot of 77 positions made by passes, restored into a fresh model, and passes from there to 400 prompt tokens"""
    n0, n = 77, 400
    q4.set_pass_context(S)
    src = q4.Transformer(models(), kv="fp8", pass_kv8=True)
    try:
        src.generate_ids(_LONG[:n0 + 1], n0)
        snap = src.snapshot(n0)
    finally:
        src.close()
    try:
        on = _run(q4, models(), _LONG[:n], bound=S, reuse=snap)
    finally:
        snap.close()
    assert on["passes"] == len(_passes(n, n + GEN, S, start=n0))
    _assert_same(_off(q4, models, n), on, "restored snapshot")


# ---- 4. poisoned bytes -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", POISON)
@pytest.mark.parametrize("first,n", [(40, 100), (600, 660)])
def test_poisoned_rows_prompt_pass(q4, models, pattern, first, n):
    """every byte of rows [first, seq_len) of both caches poisoned behind a warm run, then passes from `first` upward (a one-pass stretch; a split
    stretch): the per-token run given the same poison, and nothing written more than PROMPT_PASS_MAX rows above where the run ends"""
    prompt = _LONG[:n]
    kw = dict(start=first, warm=prompt[:first + 1], poison=(pattern, first))
    off = _run(q4, models(), prompt, kv8=False, ingest=0, **kw)
    on = _run(q4, models(), prompt, bound=S, **kw)
    assert off["passes"] == 0 and on["passes"] == len(_passes(n, n + GEN, S, start=first)) > 0
    _assert_same(off, on, "%s from row %d" % (pattern, first), rng=False)
    _assert_same(_off(q4, models, n), on, "%s from row %d against the clean run" % (pattern, first), rng=False)


@pytest.mark.parametrize("pattern", POISON)
@pytest.mark.parametrize("p", [40, 600])
def test_poisoned_rows_verify_pass(q4, models, pattern, p):
    _verify_all_indices(q4, models(), p, 7, poison=pattern)


# ---- 5. compositions ---------------------------------------------------------------------------------------------------------------------------------------------
def test_with_pass_gqa(q4, models):
    """gqa7b_pair: both switches on, 700 prompt tokens through the one-pass and both split stretches"""
    off = _off(q4, models, 700, name=GQA)
    on = _run(q4, models(GQA), _LONG[:700], bound=S, pass_gqa=True)
    assert on["passes"] == len(_passes(700, 706, S)) > 80
    _assert_same(off, on, "gqa7b_pair, 700 prompt tokens")
    only = _run(q4, models(GQA), _LONG[:41], pass_gqa=False)
    assert only["passes"] == 0, "a grouped-query FP8 model needs q4_set_pass_gqa too"


def test_score_ids_by_passes(q4, models):
    tokens = _prompt(251, seed=9)
    res = {}
    for on in (False, True):
        t = q4.Transformer(models(), kv="fp8", logprobs=5, pass_logprobs=on, pass_kv8=on)
        try:
            res[on] = _score(q4, t, tokens, 5)
            res[on]["blob"] = _blob(t, t.pos())
        finally:
            t.close()
    off, on = res[False], res[True]
    assert off["passes"] == 0 and on["passes"] == 250 // T + 1
    assert on["lp"] == off["lp"] and np.isfinite(np.frombuffer(on["lp"], dtype=np.float32)).all()
    assert np.array_equal(on["logits"], off["logits"]) and on["pos"] == off["pos"] == 250
    assert on["records"] == off["records"] and on["blob"] == off["blob"]


def test_verify_pass_with_records(q4, models):
    want = _stepwise(q4, models(), 30, logprobs=5)
    R = want["R"]
    ref_t = q4.Transformer(models(), kv="fp8", logprobs=5)
    t = q4.Transformer(models(), kv="fp8", logprobs=5, pass_logprobs=True, pass_kv8=True)
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
        assert _blob(t, 34) == want["blobs"][3]
    finally:
        q4.lib().q4_set_prompt_ingest(T)
        t.close()
        ref_t.close()


def test_sampled_verify_passes(q4, models):
    """the sampled verify pass: tokens, bytes, logits and rng_state of the run without speculation"""
    kw = dict(temperature=0.5, topp=0.6, seed=7, steps=17 + 280)
    off = _run(q4, models(), _prompt(17), kv8=False, ingest=0, **kw)
    assert len(off["tokens"]) == 17 + 280 + 1, "the off run meets an EOS: choose another seed"
    on = _run(q4, models(), _prompt(17), drafter=tsg.DRAFTERS["alternating"](off["tokens"]), speculative=dict(draft=4, sampled=True), **kw)
    print("sampled: passes, drafted, accepted = %s" % (on["stats"],))
    assert on["stats"][0] >= 10 and 0 < on["stats"][2] < on["stats"][1], on["stats"]
    _assert_same(off, on, "sampled, alternating drafter")


def test_with_logit_stages(q4, models):
    """q4_set_pass_stages with top-k 40 and a repeat penalty: verify passes run the stages' row forms"""
    kw = dict(sampling=dict(top_k=40, repeat_penalty=1.3), steps=17 + 200)
    off = _run(q4, models(), _prompt(17), kv8=False, ingest=0, **kw)
    assert len(off["tokens"]) == 17 + 200 + 1, "the off run meets an EOS: choose another seed"
    on = _run(q4, models(), _prompt(17), drafter=tsg.DRAFTERS["alternating"](off["tokens"]), spec=dict(draft=4, ngram=3, min=1), pass_stages=True, **kw)
    print("stages: passes, drafted, accepted = %s" % (on["stats"],))
    assert on["stats"][0] >= 10 and on["stats"][2] > 0, on["stats"]
    _assert_same(off, on, "top-k 40 + repeat penalty")


# ---- 6. hostile weights -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("trait", ["massive", "quant_edges"])
def test_hostile_weights(q4, models, trait):
    """massive residual channels (rows whose exponent sits at the top of the range), and pinned zero points / q == z groups / scales over two decades:
    17 prompt tokens by passes, and q4_verify_tokens at position 30 at every first-wrong index"""
    path = models(NAME, trait)
    off = _off(q4, models, 2 * T + 1, trait=trait)
    on = _run(q4, path, _LONG[:2 * T + 1])
    assert on["passes"] == 2
    _assert_same(off, on, "%s, 17 prompt tokens" % trait)
    _verify_all_indices(q4, path, 30, 7)
