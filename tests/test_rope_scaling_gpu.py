"""RoPE scaling on synthetic models (q4_set_rope_scaling; Transformer(path, rope_scaling=...)): the table the model builds, the setting's way into every
per-token path at every fusion level and with the FP8 cache, the whole scaled forward against the oracle, snapshots, context shift, the process-wide
setting's lifetime and the CLI."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import context_shift_ref as shift_ref
import rope_scaling_ref as ref
from conftest import GOLDEN, ROOT
from llama_cu_awq_amd import synth
from test_forward_gpu import BOUND, _logit_close

pytestmark = pytest.mark.gpu
ERR_ARG = 5
EXE = os.path.join(ROOT, "llama_cu_awq_amd", "bin", "llama2_q4")
TOK = os.path.join(GOLDEN, "tokenizer.bin")
MICRO = os.path.join(GOLDEN, "micro_model.bin")
SEED = 7
LINEAR1, LINEAR2, LINEAR4 = ({"type": "linear", "factor": f} for f in (1.0, 2.0, 4.0))
# Llama-3's rule with an original context of 64 positions: all three bands are populated at head 128 / theta 1e4 (and at head 64)
LLAMA3_64 = {"rope_type": "llama3", "factor": 8.0, "low_freq_factor": 1.0, "high_freq_factor": 4.0, "original_max_position_embeddings": 64}
LLAMA3_IDENTITY = dict(LLAMA3_64, original_max_position_embeddings=2 ** 30)       # every pair in the high band
PROMPT = [1, 17, 300, 45, 9]
STEPS = 12


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("rope_scaling")
    made = {}

    def get(name, theta=None):
        if name == "micro":
            return MICRO
        key = (name, theta)
        if key not in made:
            cfg = list(synth.geometry(name))
            if theta is not None:
                cfg[7] = theta
            path = str(d / ("%s_%s.bin" % (name, "own" if theta is None else "%g" % theta)))
            synth.write_model(path, tuple(cfg), seed=SEED)
            made[key] = path
        return made[key]
    return get


def head_size_of(t):
    return t.config.dim // t.config.n_heads


def table_of(t, n=None):
    """rows [0, n) of the model's rotation table: [n, head_size/2, 2] float32"""
    return np.stack([t.rope_row(p) for p in range(t.config.seq_len if n is None else n)])


def run_steps(q4, t, prompt, steps, rows_of_layer0=False):
    """the stepwise loop of test_forward_logits_and_kv: (logit bits per position, token ring[, layer 0's K / V rows])"""
    t.reset(prompt)
    logits = []
    for pos in range(steps):
        t.run_transformer(pos >= len(prompt) - 1)
        q4.synchronize()
        logits.append(t.logits().view(np.uint16).copy())
    q4.check(q4.lib().q4_handoff_status(t.state))
    ring = [int(t.token(i)) for i in range(steps + 1)]
    if rows_of_layer0:
        return np.stack(logits), ring, np.stack([np.stack(t.kv_row(0, p)) for p in range(steps)]).view(np.uint16)
    return np.stack(logits), ring


def at_level(q4, fusion, fn):
    L = q4.lib()
    L.q4_set_fusion(fusion)
    try:
        return fn()
    finally:
        L.q4_set_fusion(q4.DEFAULT_FUSION)


# ---- 1. the table ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["micro", "head128"])
def test_table(q4, files, observed, name):
    path = files(name)
    plain, one, two, l3 = (q4.Transformer(path, rope_scaling=s) for s in (None, LINEAR1, LINEAR2, LLAMA3_64))
    try:
        hs, theta, n = head_size_of(plain), plain.config.rope_theta, plain.config.seq_len
        for t, scaling in ((one, LINEAR1), (two, LINEAR2), (l3, LLAMA3_64)):
            want = q4.rope_inv_freq(scaling, hs, theta)
            assert np.array_equal(t.rope_inv_freq().view(np.uint32), want.view(np.uint32))
            assert ref.ulp_diff32(want, ref.inv_freq32(scaling, hs, theta)).max() <= 1
        assert two.rope_scaling == {"rope_type": "linear", "factor": 2.0} and l3.rope_scaling == LLAMA3_64 and plain.rope_scaling is None
        tabs = {k: table_of(t) for k, t in (("plain", plain), ("one", one), ("two", two), ("l3", l3))}
        # float(2p) * (f / 2) == float(p) * f exactly: row 2p under factor 2 is row p under factor 1, bit for bit
        half = (n + 1) // 2
        assert np.array_equal(tabs["two"][0:2 * half:2].view(np.uint32), tabs["one"][:half].view(np.uint32))
        assert not np.array_equal(tabs["two"][1], tabs["one"][1])
        assert np.array_equal(tabs["one"][0], np.stack([np.ones(hs // 2), np.zeros(hs // 2)], axis=1))

        # accuracy: every table against float64 (cos, sin) of ITS fp32 product. The unscaled table's frequencies are 1 / powf on the device, known here up
        # to an ulp or two: of the neighbours of numpy's fp32 value the one the column fits best is taken as the frequency the device used
        def worst(table, freq32):
            return np.abs(table.astype(np.float64) - ref.table64(freq32, range(n))).max(axis=(0, 2))         # per pair
        i = np.arange(hs // 2)
        f0 = (np.float32(1.0) / np.power(np.float32(theta), ((i * 2) % hs).astype(np.float32) / np.float32(hs), dtype=np.float32)).astype(np.float32)
        cands = [f0]
        for direction in (np.float32(0.0), np.float32(np.inf)):
            f = f0
            for _ in range(3):
                f = np.nextafter(f, direction).astype(np.float32)
                cands.append(f)
        own = float(np.min([worst(tabs["plain"], f) for f in cands], axis=0).max())
        figures = {"unscaled": own}
        for key, tab, t in (("linear1", "one", one), ("linear2", "two", two), ("llama3_orig64", "l3", l3)):
            figures[key] = float(worst(tabs[tab], t.rope_inv_freq()).max())
        observed.setdefault("rope_scaling_table_worst_abs_deviation_from_float64", {})[name] = figures
        print("table deviation from float64, %s: %r" % (name, figures))
        assert 0.0 < own < 1e-6
        for key in ("linear1", "linear2", "llama3_orig64"):
            assert figures[key] <= 2.0 * own, (key, figures)         # the same cosf / sinf; the factor two covers the argument-dependent spread
    finally:
        for t in (plain, one, two, l3):
            t.close()


# ---- 2. the setting reaches the per-token path, exactly ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, fusion, kv", [("tiny", 5, "fp16"), ("tiny", 1, "fp16"), ("tiny", 0, "fp16"), ("tiny", 5, "fp8"), ("tiny", 0, "fp8"),
                                              ("tiny_gqa", 5, "fp16"), ("tiny_gqa", 1, "fp16"), ("tiny_gqa", 0, "fp16")])
def test_layer0_rows_at_doubled_positions(q4, files, name, fusion, kv):
    """layer 0's K / V rows depend on the token and the position only: position 2p under factor 2 rotates like position p under factor 1. (tiny_gqa's
    heads of 32 have no FP8 cache.)"""
    rng = np.random.default_rng(5)
    b_tokens = np.concatenate([[1], rng.integers(3, 512, 7)]).astype(np.int32)
    a_tokens = rng.integers(3, 512, 15).astype(np.int32)
    a_tokens[0::2] = b_tokens

    def run():
        rows = []
        for scaling, tokens in ((LINEAR2, a_tokens), (LINEAR1, b_tokens)):
            t = q4.Transformer(files(name), kv=kv, rope_scaling=scaling)
            try:
                t.reset(tokens)
                for _ in range(len(tokens)):
                    t.run_transformer(False)
                q4.synchronize()
                rows.append(np.stack([np.stack(t.kv_row(0, p)) for p in range(len(tokens))]).view(np.uint16))
            finally:
                t.close()
        return rows
    a, b = at_level(q4, fusion, run)
    assert np.array_equal(a[0::2], b)
    assert not np.array_equal(a[2, 0], a[1, 0]) and b[:, 0].any()


# ---- 3. the whole scaled forward against the oracle ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def oracle_runs():
    """the oracle's logits of a model file along a token sequence, computed once and shared by the fusion levels (which feed the same tokens unless a
    near-tie resolves the other way: then the sequence is run again)"""
    state = {}

    def logits(orc, path, toks, pos):
        m, fed, out = state.get(path, (None, [], []))
        if m is None or fed[:min(len(fed), pos + 1)] != list(toks[:min(len(fed), pos + 1)]):
            if m is not None:
                m.close()
            m, fed, out = orc.Model(path), [], []
        while len(fed) <= pos:
            out.append(m.forward(int(toks[len(fed)]), len(fed)))
            fed.append(int(toks[len(fed)]))
        state[path] = (m, fed, out)
        return out[pos]
    yield logits
    for m, _, _ in state.values():
        m.close()


@pytest.mark.parametrize("name", ["tiny_gqa", "head128"])
@pytest.mark.parametrize("fusion", [5, 3, 1, 0])
def test_custom_frequencies_of_another_theta_match_the_oracle(q4, orc, files, oracle_runs, name, fusion):
    """the same weights under header theta 1e4 and 5e5; the 1e4 file opened with theta 5e5's frequencies as CUSTOM must be the oracle's forward of the
    5e5 file: logits of every position (q included, through the attention) and the K / V rows, under test_forward_logits_and_kv's bounds and near-tie rule"""
    lo, hi = files(name, 1e4), files(name, 5e5)
    a, b = np.fromfile(lo, dtype=np.uint8), np.fromfile(hi, dtype=np.uint8)
    assert a.shape == b.shape and np.array_equal(np.nonzero(a != b)[0] // 4 * 4, np.full(np.count_nonzero(a != b), 28)) and (a != b).any()
    hs = synth.geometry(name)[0] // synth.geometry(name)[3]
    L = q4.lib()

    def run():
        t = q4.Transformer(lo, rope_scaling={"kind": "custom", "inv_freq": q4.rope_inv_freq(None, hs, 5e5)})
        try:
            assert t.config.rope_theta == 1e4 and t.rope_scaling["kind"] == "custom"
            t.reset(PROMPT)
            toks = list(PROMPT)
            for pos in range(STEPS):
                gen = pos >= len(PROMPT) - 1
                t.run_transformer(gen)
                q4.synchronize()
                want = oracle_runs(orc, hi, toks, pos)
                got = t.logits()
                assert _logit_close(got, want, BOUND[name]).all(), "pos %d: max |d| %g" % (pos, np.abs(got.astype(np.float32) - want.astype(np.float32)).max())
                assert t.pos() == pos + 1
                if gen:
                    nxt = t.token(pos + 1)
                    top2 = np.sort(want.astype(np.float32))[-2:]
                    if top2[1] - top2[0] > 4e-3 * max(1.0, abs(top2[1])):      # not a near-tie
                        assert nxt == int(np.argmax(want.astype(np.float32))), pos
                    toks.append(nxt)
            q4.check(L.q4_handoff_status(t.state))
        finally:
            t.close()
    at_level(q4, fusion, run)


# ---- 4. Llama-3's rule, non-identity ---------------------------------------------------------------------------------------------------------------------
def test_llama3_levels_agree_and_differ_from_the_unscaled_model(q4, files):
    path = files("head128")
    assert [len(b) for b in ref.llama3_bands(LLAMA3_64, 128, 1e4)] == [7, 10, 47]       # all three bands at head 128

    def run(fusion, scaling):
        def go():
            t = q4.Transformer(path, rope_scaling=scaling)
            try:
                return run_steps(q4, t, PROMPT, STEPS, rows_of_layer0=True)
            finally:
                t.close()
        return at_level(q4, fusion, go)
    l0, l1, l3, plain = run(0, LLAMA3_64), run(1, LLAMA3_64), run(3, LLAMA3_64), run(1, None)
    assert l0[1] == l1[1] and np.array_equal(l0[0], l1[0]) and np.array_equal(l0[2], l1[2])        # levels 1 and 0: bit for bit
    assert l3[1] == l1[1], "token rings differ (levels 3 and 1)"
    af, bf = l3[0].view(np.float16).astype(np.float64), l1[0].view(np.float16).astype(np.float64)
    assert np.isfinite(af).all() and float((np.abs(af - bf) / np.maximum(1.0, np.abs(bf))).max()) <= BOUND["head128"]
    assert np.array_equal(l3[2], l1[2])                                                            # (layer 0's rows come from the same QKV launch)
    assert np.array_equal(plain[0][0], l1[0][0]) and np.array_equal(plain[2][0], l1[2][0])        # position 0 rotates by nothing under any setting
    assert any(not np.array_equal(plain[0][p], l1[0][p]) for p in range(1, STEPS))
    n = len(PROMPT)                                                                                # (the prompt's positions: the same tokens in both)
    assert all(not np.array_equal(plain[2][p, 0], l1[2][p, 0]) for p in range(1, n)) and np.array_equal(plain[2][:n, 1], l1[2][:n, 1])   # K rows differ, V rows do not


def test_llama3_ffn_pair_phase_3_reads_the_same_table(q4, files):
    """levels 5 and 3 agree bit for bit on the 7B-wide two-layer model, as test_ffn_pair_gpu asserts for the unscaled one: layer 1's q / k come from the FFN
    launch's third phase at level 5, from the QKV launch at level 3"""
    path = files("ffn_pair7b")
    L = q4.lib()
    before = L.q4_handoff_timeouts()

    def run(fusion):
        def go():
            t = q4.Transformer(path, rope_scaling=LLAMA3_64)
            try:
                out = run_steps(q4, t, PROMPT, STEPS)
                rows = np.stack([np.concatenate(t.kv_row(1, p)) for p in range(STEPS)]).view(np.uint16)
                return out + (rows,)
            finally:
                t.close()
        return at_level(q4, fusion, go)
    a, b = run(3), run(5)
    assert L.q4_handoff_timeouts() == before
    assert a[1] == b[1] and np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2])
    assert np.isfinite(a[0].view(np.float16).astype(np.float32)).all()


# ---- 5. identity parameters ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tiny", "head128"])
def test_llama3_with_every_pair_in_the_high_band_is_linear_1(q4, files, name):
    outs = []
    for scaling in (LLAMA3_IDENTITY, LINEAR1):
        t = q4.Transformer(files(name), rope_scaling=scaling)
        try:
            outs.append(run_steps(q4, t, PROMPT, STEPS) + (t.rope_inv_freq(),))
        finally:
            t.close()
    assert np.array_equal(outs[0][2].view(np.uint32), outs[1][2].view(np.uint32))
    assert outs[0][1] == outs[1][1] and np.array_equal(outs[0][0], outs[1][0])


# ---- 6. snapshots ----------------------------------------------------------------------------------------------------------------------------------------
def test_snapshots_carry_the_frequencies(q4, files):
    path = files("tiny")
    prompt = np.array([1, 17, 300, 45, 9, 77, 12, 5, 401, 3, 250, 31], dtype=np.int32)
    a = q4.Transformer(path, rope_scaling=LINEAR2)
    b = q4.Transformer(path, rope_scaling="linear,factor=2")
    plain, four = q4.Transformer(path), q4.Transformer(path, rope_scaling=LINEAR4)
    try:
        full = a.generate_ids(prompt, 30)[0].copy()
        snap = a.snapshot(10)
        assert snap.info["fingerprint"] not in (0, q4.Snapshot.from_bytes(snapshot_of(q4, plain, prompt)).info["fingerprint"])
        resumed = b.generate_ids(prompt, 30, reuse=snap)[0]
        assert np.array_equal(resumed, full)
        for other in (plain, four):
            other.reset(prompt)              # (plain has run: its rows are what they are; they must stay)
            q4.synchronize()
            rows = np.stack(other.kv_row(1, 3))
            with pytest.raises(q4.Q4Error, match="status 5"):
                other.restore(snap)
            q4.synchronize()
            assert np.array_equal(np.stack(other.kv_row(1, 3)).view(np.uint16), rows.view(np.uint16))
        snap.close()
    finally:
        for t in (a, b, plain, four):
            t.close()


def snapshot_of(q4, t, prompt):
    t.generate_ids(prompt, 14)
    s = t.snapshot(10)
    blob = s.to_bytes()
    s.close()
    return blob


# ---- 7. context shift --------------------------------------------------------------------------------------------------------------------------------------
def test_context_shift_rotates_by_the_scaled_table(q4, files):
    n_pos, keep, D = 40, 3, 11
    t, plain = q4.Transformer(files("tiny"), rope_scaling=LLAMA3_64), q4.Transformer(files("tiny"))
    try:
        t.generate_ids(PROMPT, n_pos)
        assert t.pos() == n_pos
        layers, hs = t.config.n_layers, head_size_of(t)
        k = np.stack([np.stack([t.kv_row(l, p)[0] for p in range(n_pos)]) for l in range(layers)])
        v = np.stack([np.stack([t.kv_row(l, p)[1] for p in range(n_pos)]) for l in range(layers)])
        row = t.rope_row(D)
        assert not np.array_equal(row, plain.rope_row(D))                       # the scaled table's row, not rope_theta's
        assert np.abs(row.astype(np.float64) - ref.table64(t.rope_inv_freq(), [D])[0]).max() < 1e-6     # ... of D positions at the scaled frequencies
        shift_ref.shift_fp16(k, v, n_pos, keep, D, hs, row)
        t.shift_context(keep, D)
        assert t.pos() == n_pos - D
        for l in range(layers):
            for p in range(n_pos - D):
                gk, gv = t.kv_row(l, p)
                assert np.array_equal(gk.view(np.uint16), k[l, p].view(np.uint16)) and np.array_equal(gv.view(np.uint16), v[l, p].view(np.uint16)), (l, p)
    finally:
        t.close()
        plain.close()


# ---- 8. the process-wide setting does not leak -------------------------------------------------------------------------------------------------------------
def test_the_setting_lives_for_one_build(q4, files):
    L = q4.lib()
    path = files("tiny")

    def current():
        r = q4.RopeScaling()
        q4.check(L.q4_get_rope_scaling(C.byref(r)))
        return r.kind
    first = q4.Transformer(path)
    rows = table_of(first)
    scaled = q4.Transformer(path, rope_scaling=LLAMA3_64)
    assert current() == q4.ROPE_NONE                         # restored right behind the build
    info = q4.RopeScaling()
    q4.check(L.q4_rope_scaling_of(scaled.h, C.byref(info)))
    assert info.kind == q4.ROPE_LLAMA3 and info.original_max_position == 64 and bool(info.inv_freq)
    assert not np.array_equal(table_of(scaled), rows)
    scaled.close()
    assert current() == q4.ROPE_NONE
    second = q4.Transformer(path)
    try:
        assert np.array_equal(table_of(second).view(np.uint32), rows.view(np.uint32))
        out = np.zeros(head_size_of(second) // 2, dtype=np.float32)
        assert L.q4_get_rope_inv_freq(second.h, out.ctypes.data) == ERR_ARG and second.rope_scaling is None
        q4.check(L.q4_rope_scaling_of(second.h, C.byref(info)))
        assert info.kind == q4.ROPE_NONE and not info.inv_freq
        with pytest.raises(q4.Q4Error, match="custom frequencies"):
            q4.Transformer(path, rope_scaling={"kind": "custom", "inv_freq": np.ones(16, dtype=np.float32)})       # head 64 needs 32
        assert current() == q4.ROPE_NONE
        with pytest.raises(ValueError):
            q4.Transformer(path, rope_scaling={"type": "linear", "factor": 0.5})
        assert current() == q4.ROPE_NONE
        # a process-wide setting made by hand is what a default Transformer() replaces for its build and puts back
        q4.check(L.q4_set_rope_scaling(C.byref(q4.rope_scaling_struct(LINEAR4)[0])))
        third = q4.Transformer(path)
        assert current() == q4.ROPE_LINEAR and third.rope_scaling is None
        assert np.array_equal(table_of(third, 8).view(np.uint32), rows[:8].view(np.uint32))
        third.close()
    finally:
        L.q4_set_rope_scaling(None)
        first.close()
        second.close()


# ---- 9. the CLI ------------------------------------------------------------------------------------------------------------------------------------------------
def _cli(setting):
    env = {k: v for k, v in os.environ.items() if k != "Q4_ROPE_SCALING"}
    if setting is not None:
        env["Q4_ROPE_SCALING"] = setting
    return subprocess.run([EXE, MICRO, "-z", TOK, "-n", "32", "-t", "0"], capture_output=True, timeout=300, env=env)


def _printed(q4, tokens):
    """what generate() prints for a token ring: the pieces, single bytes only where printable (safe_printf)"""
    tk = q4.Tokenizer(TOK, 128)
    out = b""
    for prev, tok in zip(tokens[:-1], tokens[1:]):
        piece = tk.decode(int(prev), int(tok)) or b""
        if len(piece) == 1 and not (32 <= piece[0] < 127 or piece in b"\t\n\v\f\r"):
            continue
        out += piece
    tk.close()
    return out


def test_cli_reads_the_environment_variable(q4):
    strip = lambda b: b[:b.index(b"achieved tok/s")]
    generated = lambda b: b.split(b"Encoding Prompt... Done!\n", 1)[1].split(b"\n\nachieved tok/s", 1)[0]
    plain, none, scaled = _cli(None), _cli("none"), _cli("linear,factor=2")
    assert plain.returncode == 0 and none.returncode == 0 and scaled.returncode == 0, (plain.stderr, scaled.stderr)
    assert b"rope_scaling" not in plain.stdout and strip(plain.stdout) == strip(none.stdout) == strip(_cli("").stdout)
    assert b"rope_theta: 10000\nrope_scaling: linear,factor=2\n" in scaled.stdout
    for out, scaling in ((scaled, "linear,factor=2"), (plain, None)):
        t = q4.Transformer(MICRO, rope_scaling=scaling)
        toks = t.generate_ids([1], 32)[0]
        t.close()
        assert len(toks) == 33 and generated(out.stdout) == _printed(q4, toks[:32])      # (-n 32 prints the tokens of positions 1 .. 31)
        assert b"Tokens: 31," in out.stdout
    l3 = _cli("llama3,factor=8,low=1,high=4,orig=8192")
    assert l3.returncode == 0 and b"rope_scaling: llama3,factor=8,low=1,high=4,orig=8192\n" in l3.stdout
    for bad in ("linear", "linear,factor=0.5", "yarn,factor=4", "llama3,factor=8"):
        r = _cli(bad)
        assert r.returncode != 0 and b"Q4_ROPE_SCALING" in r.stderr and b"llama3,factor=8,low=1,high=4,orig=8192" in r.stderr, bad
