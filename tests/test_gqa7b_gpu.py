"""Grouped-query attention at 7B width: `gqa7b_pair`, the Mistral-7B / Llama-3-8B layer twice (dim 4096, hidden 14336, 32 query heads over 8 K / V heads,
head 128, rope_theta 5e5) with a context of 2304, so every graph bin up to 4096 runs with kv_mul = 4 inside the network:

  bins 128 / 256 ........ the attention -> o-proj launch on sixteen-wave blocks (layer_attn.hip ao16_takes: K = dim = 4096, head 128, V-slice forms 5 / 6)
  bins 512 / 1024 / 2048  its split-context forms in chunks of 64 / 128 / 256 positions (forms 4 / 2 / 3), merged by each head's last block
  bin 4096 .............. eighteen chunks of 256 at positions 2048 .. 2303: the merge's two-round branch
  hidden 14336 .......... gate / up (N = 14336) and down (K = 14336) as strips behind the in-launch hand-offs; the FFN pair launch does not cover this hidden
                          size (q4_ffn_pair_covers == 0), so levels 4 and 5 run level 3's launches here
  FP8 cache ............. the stand-alone kv8 attention with kv_mul = 4 at head 128

against the CPU restatement (oracle.Model), the unrounded double forward, kv8_ref's composed forward, and the fusion levels against each other. Every worst
value goes through `observed` (committed copy: profiles/gqa7b_parity_observed.json)."""
import numpy as np
import pytest

import kv8_ref
from llama_cu_awq_amd import synth
from test_baseline_configs_gpu import _kv_to_host, _rel, _rms

pytestmark = pytest.mark.gpu

NAME = "gqa7b_pair"
SEED = 7
TOKENS = [1, 17, 300, 45, 9, 33, 2, 400, 77, 12, 250, 5]
LEVELS_GRAPHS = [(5, 1), (3, 1), (1, 1), (0, 1), (3, 0), (1, 0), (0, 0)]
BOUND = 5e-3                      # tests/test_ffn_pair_gpu.py's bound for the two-layer 4096-wide model; the restatement sits 6.28e-3 from the double forward here, 6.69e-3 there
CHECKPOINTS = (3, 127, 128, 255, 256, 300, 511, 512, 600, 1023, 1024, 1500, 2047, 2048, 2299)
STEPS = 2300
SPLIT_POSITIONS = (300, 511, 512, 1023, 1024, 2100)
KV8_POSITIONS = 40
# The FP8 model against the composed forward: measured 2.0e-2 at position 25, every level and graph mode alike (profiles/gqa7b_parity_observed.json,
# gqa7b_pair / kv8_vs_composed_forward) -- above the 5e-3 that holds on tiny and head64_long. It is rounding, not the attention: with the GPU's own rows
# in the composed forward's cache the same logits lie within 4.4e-3 at all 40 positions (test_fp8_cache_one_step_from_the_gpus_own_rows; key
# kv8_one_step_from_the_gpus_rows). What is left is K / V elements that round to the other e4m3 neighbour in one of the two evaluations -- 2.3 % of layer
# 1's at 1024 elements per row -- which every later position reads. The bound is twice the measured value.
KV8_BOUND = 4.0e-2
KV8_LONG = 1100
KV8_CHECKPOINTS = (511, 512, 1023, 1024, 1099)


def _forced_tokens(n, seed=3):
    return [1] + [int(v) for v in np.random.default_rng(seed).integers(3, 512, size=n - 1)]


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    p = str(tmp_path_factory.mktemp("gqa7b") / (NAME + ".bin"))
    synth.write_model(p, NAME, seed=SEED)
    return p


@pytest.fixture(scope="module")
def restatement(orc, model):
    """TOKENS through the restatement and the unrounded double forward, once: (logits f16 [12, vocab], K rows, V rows [layers, 12, kv_dim], f64 logits)"""
    m = orc.Model(model)
    logits = np.stack([m.forward(tok, pos) for pos, tok in enumerate(TOKENS)])
    k, v = m.kv()
    k, v = k[:, :len(TOKENS)].copy(), v[:, :len(TOKENS)].copy()
    m.close()
    m = orc.Model(model)
    f64 = np.stack([m.forward_f64(tok, pos, cap=len(TOKENS)) for pos, tok in enumerate(TOKENS)])
    m.close()
    return logits, k, v, f64


def _rec(observed, key):
    return observed.setdefault(NAME, {}).setdefault(key, {})


# ---- a. lockstep with the restatement -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fusion,graphs", LEVELS_GRAPHS)
def test_lockstep_with_the_restatement(q4, model, restatement, observed, fusion, graphs):
    """Twelve forced positions at every level and graph mode: logits within 5e-3 of the restatement and inside the bracket around the unrounded double
    forward at every position, K / V rows of both layers at positions 0 and 11 within 3e-3. (Bin 128: the V-slice form 5 on sixteen-wave blocks at levels
    3 / 5, the stand-alone launches at levels 1 / 0; gate / up and down as strips.)"""
    L = q4.lib()
    ref, rk, rv, f64 = restatement
    rec = _rec(observed, "lockstep_f%d_g%d" % (fusion, graphs))
    before = L.q4_handoff_timeouts()
    L.q4_set_fusion(fusion)
    L.q4_set_use_graphs(graphs)
    try:
        t = q4.Transformer(model)
        t.reset(TOKENS)
        worst = wg = wr = 0.0
        for pos in range(len(TOKENS)):
            t.run_transformer(pos >= len(TOKENS) - 1)
            q4.synchronize()
            got = t.logits()
            assert np.isfinite(got.astype(np.float32)).all(), pos
            e = _rel(got, ref[pos])
            eg, er = _rel(got, f64[pos]), _rel(ref[pos], f64[pos])
            rg, rr = _rms(got, f64[pos]), _rms(ref[pos], f64[pos])
            worst, wg, wr = max(worst, e), max(wg, eg), max(wr, er)
            print("fusion %d graphs %d pos %2d: vs restatement %.3e; vs f64 gpu %.3e restatement %.3e; rms gpu %.3e restatement %.3e" % (fusion, graphs, pos, e, eg, er, rg, rr))
            assert e <= BOUND, "pos %d: max rel logit err %g vs the restatement" % (pos, e)
            assert eg <= 2.0 * er + 1e-3, "pos %d: GPU %g vs restatement %g from the unrounded forward" % (pos, eg, er)
            assert rg <= 1.5 * rr + 1e-4, "pos %d: rms distance from the unrounded forward, GPU %g vs restatement %g" % (pos, rg, rr)
            assert t.pos() == pos + 1
        rec.update({"logits_max_rel_vs_restatement": worst, "vs_f64_gpu_max": wg, "vs_f64_restatement_max": wr, "bound": BOUND})
        wkv = 0.0
        for layer in range(t.config.n_layers):
            for pos in (0, len(TOKENS) - 1):
                gk, gv = t.kv_row(layer, pos)
                ek, ev = _rel(gk, rk[layer, pos]), _rel(gv, rv[layer, pos])
                wkv = max(wkv, ek, ev)
                assert ek <= 3e-3 and ev <= 3e-3, (layer, pos, ek, ev)
        rec["kv_max_rel"] = wkv
        q4.check(L.q4_handoff_status(t.state))
        assert L.q4_get_fusion() == fusion and L.q4_handoff_timeouts() == before
        t.close()
    finally:
        L.q4_set_fusion(q4.DEFAULT_FUSION)
        L.q4_set_use_graphs(1)


# ---- b. every bin, the fusion levels against each other ---------------------------------------------------------------------------------------------------
def test_every_bin_fusion_levels_against_each_other(q4, model, observed):
    """2300 greedy steps through the bins 128 .. 4096 at levels 5 / 4 / 3 / 1 / 0. Levels 0 and 1: the same bits (K = 4096 has no shared half slot). Levels
    3 / 4 / 5: the same bits -- the pair launch does not cover hidden 14336, so 4 and 5 run level 3's launches and their equality says only
    that the level switch itself changes nothing. Level 3 against level 1: the rule of test_in_launch_handoffs_reproduce_the_launch_sequence_bits."""
    L = q4.lib()
    dim, hidden = synth.GEOMETRIES[NAME][:2]
    rec = _rec(observed, "levels")
    rec["ffn_pair_covers_hidden_14336"] = int(L.q4_ffn_pair_covers(dim, hidden))
    before = L.q4_handoff_timeouts()
    outs, launches = {}, {}
    t = q4.Transformer(model)
    try:
        for level in (5, 4, 3, 1, 0):
            L.q4_set_fusion(level)
            t.reset([1, 5, 9])
            got = []
            for pos in range(STEPS):
                t.run_transformer(pos >= 2)
                if pos in CHECKPOINTS:
                    q4.synchronize()
                    got.append(t.logits().view(np.uint16).copy())
            q4.synchronize()
            q4.check(L.q4_handoff_status(t.state))
            assert L.q4_get_fusion() == level and L.q4_handoff_timeouts() == before, level
            outs[level] = (got, [int(t.token(i)) for i in range(STEPS + 1)])
            # launches per layer of one eager step at position 200 (one attention -> o-proj launch from level 3 on; the FFN half as gate/up + down strips)
            t.reset([1, 5, 9])
            for pos in range(200):
                t.run_transformer(pos >= 2)
            q4.synchronize()
            launches[level] = t.bench_in_network(1 | 2 | 4 | 8 | 16, tokens=1)[3] // t.config.n_layers
    finally:
        L.q4_set_fusion(q4.DEFAULT_FUSION)
        t.close()
    rec["launches_per_layer_at_position_200"] = {str(k): v for k, v in launches.items()}
    print("q4_ffn_pair_covers(%d, %d) = %d; launches per layer at position 200 by level: %s" % (dim, hidden, rec["ffn_pair_covers_hidden_14336"], launches))
    assert launches[5] == launches[4] == launches[3] < launches[1], launches     # (attention and o-proj are ONE launch from level 3 on; no pair launch at 4 / 5)
    for got, _ in outs.values():
        assert all(np.isfinite(g.view(np.float16).astype(np.float32)).all() for g in got)
    assert outs[0][1] == outs[1][1], "token ring differs at fusion level 0"
    for a, b, pos in zip(outs[0][0], outs[1][0], CHECKPOINTS):
        assert np.array_equal(a, b), "logits differ at position %d (fusion 0 vs 1)" % pos
    for level in (4, 5):
        assert outs[level][1] == outs[3][1], "token ring differs (level %d vs 3)" % level
        for a, b, pos in zip(outs[level][0], outs[3][0], CHECKPOINTS):
            assert np.array_equal(a, b), "logits differ at position %d (level %d vs 3)" % (pos, level)
    first_div = next((i for i, (x, y) in enumerate(zip(outs[1][1], outs[3][1])) if x != y), None)
    rec["fusion3_vs_1_first_token_divergence"] = first_div
    print("first token divergence, level 3 vs 1: %s" % first_div)
    errs = {}
    for a, b, pos in zip(outs[1][0], outs[3][0], CHECKPOINTS):
        if first_div is not None and pos >= first_div:
            break
        errs[pos] = _rel(a.view(np.float16), b.view(np.float16))
        print("level 3 vs 1 at position %4d: %.3e" % (pos, errs[pos]))
    rec["fusion3_vs_1"] = {str(k): v for k, v in errs.items()}
    assert first_div is None or first_div >= 128, "token rings diverged at %d (fusion 3 vs 1)" % first_div
    for pos, err in errs.items():
        assert err <= (5e-3 if pos <= 128 else 1.2e-2), (pos, err)


# ---- c. one step from the GPU's own cache -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("level", [3, 1])
@pytest.mark.parametrize("target", [200, 400, 900, 1100, 2100])
def test_one_step_from_the_gpus_own_cache(q4, orc, model, observed, target, level):
    """tests/test_baseline_configs_gpu.py's _step_from_the_gpus_cache on this model: decode to `target` through the captured graphs, hand the GPU's cache to
    the restatement, compare the next step from the identical state -- every cached position of both layers takes part. 200: bin 256, form 6 on sixteen-wave
    blocks; 400 / 900 / 1100: split context in chunks of 64 / 128 / 256; 2100: bin 4096, the two-round merge. Level 1: the stand-alone attention."""
    L = q4.lib()
    rec = _rec(observed, "own_cache_f%d_pos%d" % (level, target))
    before = L.q4_handoff_timeouts()
    L.q4_set_fusion(level)
    try:
        t = q4.Transformer(model)
        m = orc.Model(model)
        toks, tps, timed, _ = t.generate_ids([1, 5, 9], target)
        assert timed == target - 1 and t.pos() == target
        k, v = _kv_to_host(q4, t)
        n = k.shape[0]
        np.ctypeslib.as_array(m.L.orc_key_cache(m.h), shape=(n,))[:] = k
        np.ctypeslib.as_array(m.L.orc_value_cache(m.h), shape=(n,))[:] = v
        tok = int(t.token(target))
        t.run_transformer(True)
        q4.synchronize()
        got = t.logits()
        ref = m.forward(tok, target)
        assert t.pos() == target + 1 and np.isfinite(got.astype(np.float32)).all()
        rk, rv = m.kv()
        for layer, ktol, vtol in ((0, 8e-3, 3e-3), (1, 2.4e-2, 1.2e-2)):
            gk, gv = t.kv_row(layer, target)
            ek, ev = _rel(gk, rk[layer, target]), _rel(gv, rv[layer, target])
            rec["layer%d_k_max_rel" % layer], rec["layer%d_v_max_rel" % layer] = ek, ev
            print("level %d target %d layer %d: K %.3e V %.3e" % (level, target, layer, ek, ev))
            assert ek <= ktol and ev <= vtol, (layer, ek, ev)
        e = _rel(got, ref)
        rec["logits_max_rel_vs_restatement"], rec["bound"] = e, BOUND
        print("level %d target %d: logits %.3e" % (level, target, e))
        assert e <= BOUND, e
        r32 = ref.astype(np.float32)
        top2 = np.sort(r32)[-2:]
        if top2[1] - top2[0] > 4e-3 * max(1.0, abs(top2[1])):
            assert int(t.token(target + 1)) == int(np.argmax(r32))
        q4.check(L.q4_handoff_status(t.state))
        assert L.q4_get_fusion() == level and L.q4_handoff_timeouts() == before
        # the launches of the next step, eager (it is handed its own size as the bin: the same form class and residency guard -- the guard counts the
        # waiting blocks, not the chunks -- with fewer chunks than the graph's bin): attention and o-proj are ONE launch at level 3 here, no fall-back
        per_layer = t.bench_in_network(1 | 2 | 4 | 8 | 16, tokens=1)[3] // t.config.n_layers
        rec["launches_per_layer_eager"] = per_layer
        assert per_layer == (4 if level == 3 else 5), (level, target, per_layer)
        t.close()
        m.close()
    finally:
        L.q4_set_fusion(q4.DEFAULT_FUSION)


# ---- d. graphs against eager in the split bins ------------------------------------------------------------------------------------------------------------
def _forced_logits(q4, path, toks, checkpoints, kv="fp16"):
    t = q4.Transformer(path, kv=kv)
    t.reset(toks)
    got = {}
    for pos in range(len(toks)):
        t.run_transformer(False)
        q4.synchronize()                    # (q4_run_transformer takes the position from the pinned word: it must be current)
        if pos in checkpoints:
            got[pos] = t.logits().astype(np.float64)
    q4.check(q4.lib().q4_handoff_status(t.state))
    t.close()
    return got


def _worst_between(a, b, checkpoints):
    worst = 0.0
    for pos in checkpoints:
        assert np.isfinite(a[pos]).all() and np.isfinite(b[pos]).all(), pos
        e = float((np.abs(a[pos] - b[pos]) / np.maximum(1.0, np.abs(b[pos]))).max())
        print("graphs vs eager at position %4d: %.3e" % (pos, e))
        worst = max(worst, e)
    return worst


def test_graphs_against_eager_in_the_split_bins(q4, model, observed):
    """The same forced tokens at level 3 through the captured graphs (the bins' chunk counts) and through eager launches (a step is handed its own size:
    other chunk counts, and the one-block form up to 510): the logits agree within the model's bound."""
    L = q4.lib()
    toks = _forced_tokens(max(SPLIT_POSITIONS) + 1)
    before = L.q4_handoff_timeouts()
    runs = {}
    L.q4_set_fusion(3)
    try:
        for graphs in (1, 0):
            L.q4_set_use_graphs(graphs)
            runs[graphs] = _forced_logits(q4, model, toks, SPLIT_POSITIONS)
        assert L.q4_get_fusion() == 3 and L.q4_handoff_timeouts() == before
    finally:
        L.q4_set_fusion(q4.DEFAULT_FUSION)
        L.q4_set_use_graphs(1)
    worst = _worst_between(runs[1], runs[0], SPLIT_POSITIONS)
    _rec(observed, "split_graphs_vs_eager")["logits_max_rel"] = worst
    assert worst <= 5e-3, worst


# ---- e. the FP8 cache -------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def kv8_net(model):
    cfg = synth.geometry(NAME)
    toks = _forced_tokens(KV8_POSITIONS)
    f = kv8_ref.Forward(model, cfg, round_trip=True)
    logits = np.stack([f.forward(t, pos) for pos, t in enumerate(toks)])
    return {"toks": toks, "logits": logits, "k": f.kc[:, :len(toks)].copy(), "v": f.vc[:, :len(toks)].copy()}


def _kv8_forced_run(q4, path, toks, kv):
    t = q4.Transformer(path, kv=kv)
    assert t.kv_format == kv and q4.lib().q4_kv_format_of(t.state) == q4.KV_FORMATS[kv]
    t.reset(toks)
    logits = []
    for pos in range(len(toks)):
        t.run_transformer(False)
        q4.synchronize()
        logits.append(t.logits())
    rows = [np.concatenate(t.kv_row(0, pos)) for pos in range(len(toks))]
    q4.check(q4.lib().q4_handoff_status(t.state))
    t.close()
    return np.stack(logits), np.stack(rows)


@pytest.mark.parametrize("fusion,graphs", [(5, 1), (1, 1), (0, 0)])
def test_fp8_cache_against_the_composed_forward(q4, model, kv8_net, observed, fusion, graphs):
    """tests/test_kv8_gpu.py's network test with kv_mul = 4 at head 128: layer 0's rows are the round trip of the fp16 model's, bit for bit; the logits lie
    within KV8_BOUND of the forward composed from the oracle's ops with the round trip on."""
    L = q4.lib()
    hs = 128
    L.q4_set_fusion(fusion)
    L.q4_set_use_graphs(graphs)
    try:
        l16, r16 = _kv8_forced_run(q4, model, kv8_net["toks"], "fp16")
        l8, r8 = _kv8_forced_run(q4, model, kv8_net["toks"], "fp8")
    finally:
        L.q4_set_fusion(q4.DEFAULT_FUSION)
        L.q4_set_use_graphs(1)
    assert L.q4_get_kv_format() == q4.KV_FP16
    want = kv8_ref.round_trip(r16, hs)
    bad = np.argwhere((r8.view(np.uint16) != want.view(np.uint16)).any(axis=1)).ravel()
    assert bad.size == 0, "layer-0 K / V rows are not the round trip of the fp16 rows at positions %s" % bad[:8]
    ref = kv8_net["logits"].astype(np.float64)
    assert np.isfinite(l8.astype(np.float32)).all()
    err = np.abs(l8.astype(np.float64) - ref) / np.maximum(1.0, np.abs(ref))
    worst = float(err.max())
    print("kv8 fusion %d graphs %d: worst logit error %.3e at position %d" % (fusion, graphs, worst, int(err.max(axis=1).argmax())))
    _rec(observed, "kv8_vs_composed_forward")["f%d_g%d" % (fusion, graphs)] = worst
    assert worst <= KV8_BOUND, (worst, int(err.max(axis=1).argmax()))
    assert not np.array_equal(l8, l16)


def test_fp8_cache_one_step_from_the_gpus_own_rows(q4, model, kv8_net, observed):
    """What separates the FP8 model from the composed forward above is not the attention over the cache: a K / V element that differs by one fp16 ulp
    between the two evaluations (the GPU's GEMV against the oracle's: layer 0 too) can round to the other e4m3 neighbour, a step of 2^-3 .. 2^-4 of the
    element, and every later position reads that row. An e4m3 step is 128 fp16 ulps wide, so in layer 0 -- one GEMV behind the embedding, the two
    evaluations within one fp16 ulp -- at most one element in 128 changes its byte: below 1 % (measured 14 of 81920; layer 1, whose inputs already
    differ, 1921 of 81920). Here each position's rows of
    BOTH layers enter the composed forward's cache as the GPU left them, so both evaluations attend over identical caches at every position: the logits
    must then lie within the model's fp16 bound (5e-3, section c). The GPU's rows are held to the rows the composed forward computes at the same
    position over that same cache: section c's fp16 bounds per layer plus one spacing of the row's FP8 grid (a wrong exponent, head or row misses
    that by the size of the element; "exactly the neighbouring byte" does not follow: a GEMV output's two evaluations differ by up to 3e-3 absolute,
    several spacings of an element of 0.01)."""
    L = q4.lib()
    cfg = synth.geometry(NAME)
    toks = kv8_net["toks"]
    t = q4.Transformer(model, kv="fp8")
    try:
        t.reset(toks)
        got = []
        for pos in range(len(toks)):
            t.run_transformer(False)
            q4.synchronize()
            got.append(t.logits().astype(np.float64))
        rows = [[t.kv_row(layer, pos) for layer in range(cfg[2])] for pos in range(len(toks))]
        q4.check(L.q4_handoff_status(t.state))
    finally:
        t.close()
    assert L.q4_get_kv_format() == q4.KV_FP16
    f = kv8_ref.Forward(model, cfg, round_trip=True)
    pk, pv = kv8_net["k"], kv8_net["v"]                 # the composed forward's own rows
    worst, flipped, apart, differ = 0.0, [0, 0], [0, 0], [0, 0]
    for pos, tok in enumerate(toks):
        gk, gv = np.stack([r[0] for r in rows[pos]]), np.stack([r[1] for r in rows[pos]])
        ref = f.forward(tok, pos, rows=(gk, gv)).astype(np.float64)
        for layer in range(2):
            flipped[layer] += int((pk[layer, pos].view(np.uint16) != gk[layer].view(np.uint16)).sum() + (pv[layer, pos].view(np.uint16) != gv[layer].view(np.uint16)).sum())
        # the rows themselves, against the rows the composed forward computes at this position from the now-matching caches: what the fp16 rows of the
        # two evaluations may differ by (section c's bounds per layer) plus one spacing of the row's FP8 grid at that element
        for layer, ktol, vtol in ((0, 8e-3, 3e-3), (1, 2.4e-2, 1.2e-2)):
            for what, g, p, tol in (("K", gk[layer], f.own[0][layer], ktol), ("V", gv[layer], f.own[1][layer], vtol)):
                g64, p64 = g.astype(np.float64), p.astype(np.float64)
                grid = np.maximum(kv8_ref.step(g, 128), kv8_ref.step(p, 128))
                d = np.abs(g64 - p64)
                assert np.isfinite(g64).all() and (d <= tol * np.maximum(1.0, np.abs(p64)) + grid).all(), (
                    pos, layer, what, int(np.argmax(d - grid)), float(d.max()), float(grid[np.argmax(d - grid)]))
                apart[layer] += int((d > grid).sum())
                differ[layer] += int((d > 0).sum())
        e = float((np.abs(got[pos] - ref) / np.maximum(1.0, np.abs(ref))).max())
        print("kv8 from the GPU's rows, position %2d: %.3e" % (pos, e))
        worst = max(worst, e)
    rec = _rec(observed, "kv8_one_step_from_the_gpus_rows")
    rec["logits_max_rel"] = worst
    per_layer = 2 * len(toks) * (cfg[0] * cfg[4] // cfg[3])
    rec["elements_that_differ_from_the_composed_forward_by_layer"] = flipped
    rec["elements_per_layer"] = per_layer
    rec["elements_that_differ_from_the_rows_computed_over_the_same_cache_by_layer"] = differ
    rec["of_them_more_than_one_grid_spacing_apart_by_layer"] = apart
    print("... from the rows the composed forward computes over the GPU's cache: %s, more than one spacing of the FP8 grid apart: %s" % (differ, apart))
    print("K / V elements that differ from the composed forward's, by layer: %s of %d each" % (flipped, per_layer))
    assert flipped[0] <= 0.01 * per_layer, flipped           # (layer 1's rows come from inputs that differ by more than an ulp: recorded, not bounded)
    assert worst <= 5e-3, worst


def test_fp8_cache_graphs_against_eager_in_the_split_bins(q4, model, observed):
    L = q4.lib()
    toks = _forced_tokens(KV8_LONG)
    runs = {}
    try:
        for graphs in (1, 0):
            L.q4_set_use_graphs(graphs)
            runs[graphs] = _forced_logits(q4, model, toks, KV8_CHECKPOINTS, kv="fp8")
    finally:
        L.q4_set_use_graphs(1)
    assert L.q4_get_kv_format() == q4.KV_FP16
    worst = _worst_between(runs[1], runs[0], KV8_CHECKPOINTS)
    _rec(observed, "kv8_split_graphs_vs_eager")["logits_max_rel"] = worst
    assert worst <= 5e-3, worst


# ---- f. admission -----------------------------------------------------------------------------------------------------------------------------------------
def test_passes_are_not_admitted(q4, model):
    """Prompt and verify passes cover multi-head models with a covered FFN pair launch only (prompt_pass_covers): with prompt ingest on, the pass context
    raised to the model's and speculation on, this model takes no pass, the probe says so, and the run is byte-equal to the run with all of that off."""
    L = q4.lib()
    prompt = _forced_tokens(40, seed=5)
    steps = 100

    def run(on):
        L.q4_set_prompt_ingest(8 if on else 0)
        q4.set_pass_context(2304 if on else 256)
        t = q4.Transformer(model, **({"speculative": dict(draft=4)} if on else {}))
        try:
            passes, spec = L.q4_prompt_passes(), t.spec_stats()[0]
            covers = [int(L.q4_verify_covers(t.h, pos, 4)) for pos in (0, 40, 99, 300, 600, 1100, 2100)]
            toks = t.generate_ids(prompt, steps)[0].copy()
            q4.check(L.q4_handoff_status(t.state))
            return {"tokens": toks, "logits": t.logits().view(np.uint16).copy(), "passes": L.q4_prompt_passes() - passes,
                    "spec": t.spec_stats()[0] - spec, "covers": covers}
        finally:
            t.close()
            L.q4_set_prompt_ingest(8)
            q4.set_pass_context(256)

    on, off = run(True), run(False)
    assert on["passes"] == 0 and on["spec"] == 0, on
    assert on["covers"] == [0] * 7, on["covers"]
    assert len(on["tokens"]) >= steps
    assert np.array_equal(on["tokens"], off["tokens"]), "token rings differ"
    assert np.array_equal(on["logits"], off["logits"]), "final logits differ in %d entries" % int((on["logits"] != off["logits"]).sum())
