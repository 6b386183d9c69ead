"""The fused launches (levels 3 / 4 / 5 / 6) and the launch sequences (levels 0 / 1) on the hostile checkpoints of tests/hostile_models.py:
massive residual channels, near-one-hot attention with a sink at position 0, pinned zero points / q == z groups / scales over two decades,
norm weights with zeros and negatives, and all of them at once. Every trait on ffn_pair7b (levels 4 / 5 / 6) and head128 (the attention ->
o-proj launch, split context from bin 512), `combined` on head128_gqa, head128_k5120 (the shared half slot), tinyllama (head 64, one k-slot),
small (the unfused forms) and gqa7b_pair (grouped-query 4:1 at width 4096 on sixteen-wave blocks, hidden 14336 as strips).

  a. a fixed token sequence (the GPU's own tokens never feed back) against the restatement: every position's logits, the K / V rows of the
     first and last position, every level and graph mode; no bounded wait may run out, every output finite
  b. the same logits against the unrounded double forward at the first four positions: the HIP path at most as far from it as the bracket of
     tests/test_baseline_configs_gpu.py allows relative to the restatement
  c. long greedy runs: levels 4 / 5 / 6 equal level 3 bit for bit, level 0 equals level 1 bit for bit, level 3 against level 1 within the
     model's bound until the first near-tie divergence (tests/test_forward_gpu.py's rule)"""
import ctypes as C

import numpy as np
import pytest

import hostile_models as hm
import hostile_ref
from llama_cu_awq_amd import synth

pytestmark = pytest.mark.gpu

SEED = 5
SEQ = [1, 17, 300, 45, 9, 230, 77, 401, 12, 5, 498, 64, 33, 150]     # prompt = the first 10; the last 4 are generated steps, forced
PROMPT_LEN = 10
F64_POSITIONS = 4
MODELS = [(g, t) for g in ("ffn_pair7b", "head128") for t in hm.TRAITS] + [(g, "combined") for g in ("head128_gqa", "head128_k5120", "tinyllama", "small", "gqa7b_pair")]

# logits vs the restatement, max |d| / max(1, |logit|): the benign models' bound of tests/test_forward_gpu.py (5e-3; measured <= 1.6e-3 on massive / combined)
# unless a hostile model measured more. Those carry 3x their measured worst case (parity_observed.json "hostile_vs_restatement"): near-one-hot softmaxes,
# scales over two decades and norm weights up to 8 amplify one fp16 rounding that falls the other way; the restatement itself sits 0.004 .. 0.010 from the
# unrounded forward on these models, and test (b) holds the HIP path to that bracket at every level and graph mode
BOUND = {"ffn_pair7b/peaked": 5.5e-2,          # measured 1.77e-2 (restatement vs f64: 9.4e-3)
         "ffn_pair7b/norm_weights": 3e-2,      # measured 1.03e-2 (8.1e-3)
         "ffn_pair7b/quant_edges": 2.5e-2,     # measured 7.8e-3 (6.6e-3)
         "head128/peaked": 4.5e-2,             # measured 1.51e-2 (1.04e-2)
         "head128/norm_weights": 3e-2,         # measured 9.9e-3 (9.3e-3)
         "head128/quant_edges": 2.5e-2}        # measured 8.1e-3 (3.7e-3)
DEFAULT_BOUND = 5e-3
# K / V rows of the first and last position: tests/test_forward_gpu.py's 3e-3 (measured <= 1.2e-3 on massive / combined), 3x the measured worst elsewhere
KV_BOUND = {"ffn_pair7b/peaked": 3.5e-2,       # measured 1.12e-2
            "ffn_pair7b/quant_edges": 2.2e-2,  # measured 7.3e-3
            "ffn_pair7b/norm_weights": 1e-2,   # measured 3.4e-3
            "head128/peaked": 2.3e-2,          # measured 7.7e-3
            "head128/quant_edges": 3.7e-2,     # measured 1.23e-2
            "head128/norm_weights": 9e-3}      # measured 2.9e-3
DEFAULT_KV_BOUND = 3e-3
# greedy rings of levels 3 and 1 may part at a near-tie, but not inside the first bin (tests/test_forward_gpu.py) -- except on ffn_pair7b/peaked, where
# near-one-hot attention turns the fp32 grouping difference into a token flip early: measured first divergence 32
FIRST_DIVERGENCE = {"ffn_pair7b/peaked": 16}


def _key(g, t):
    return "%s/%s" % (g, t)


@pytest.fixture(scope="module")
def hostile(tmp_path_factory):
    d = tmp_path_factory.mktemp("hostile_net")
    out = {}
    for g, t in MODELS:
        p = str(d / ("%s_%s.bin" % (g, t)))
        hm.write_hostile_model(p, g, t, seed=SEED)
        out[g, t] = p
    return out


@pytest.fixture(scope="module")
def restatement(orc, hostile):
    """(logits [T, vocab] f16, K rows, V rows of positions 0 and T-1 per layer, f64 logits of the first positions) per model, computed once
    (tests/hostile_ref.py keeps it, for tests/test_pass_hostile_gpu.py too)."""
    def get(g, t):
        logits, (k, v), f64 = hostile_ref.restatement(orc, hostile[g, t], (g, t, SEED), SEQ, F64_POSITIONS)
        return logits, (k[:, [0, len(SEQ) - 1]], v[:, [0, len(SEQ) - 1]]), f64
    return get


def _ring(t):
    base = t.state.contents.shared_data
    return np.ctypeslib.as_array((C.c_int * t.config.seq_len).from_address(base + 4))


def _forced(q4, t):
    """SEQ through the model: prompt steps, then generated steps whose token is overwritten with SEQ's. Returns logits [T, vocab], kv rows."""
    t.reset(SEQ[:PROMPT_LEN])
    ring = _ring(t)
    out = []
    for pos in range(len(SEQ)):
        gen = pos >= PROMPT_LEN - 1
        t.run_transformer(gen)
        q4.synchronize()
        out.append(t.logits().copy())
        if gen and pos + 1 < len(SEQ):
            ring[pos + 1] = SEQ[pos + 1]
    rows = [[t.kv_row(layer, p) for p in (0, len(SEQ) - 1)] for layer in range(t.config.n_layers)]
    return np.stack(out), rows


def _levels(q4, geom):
    dim, hidden = synth.GEOMETRIES[geom][:2]
    return [0, 1, 3, 5] + ([4, 6] if q4.lib().q4_ffn_pair_covers(dim, hidden) else [])


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b) / np.maximum(1.0, np.abs(b))


def _rms(a, b):
    return float(np.sqrt(np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2)))


@pytest.mark.parametrize("geom,trait", MODELS)
def test_hostile_forward_against_the_restatement(q4, hostile, restatement, observed, geom, trait):
    L = q4.lib()
    ref, (rk, rv), f64 = restatement(geom, trait)
    assert np.isfinite(ref.astype(np.float32)).all()
    bound = BOUND.get(_key(geom, trait), DEFAULT_BOUND)
    kv_bound = KV_BOUND.get(_key(geom, trait), DEFAULT_KV_BOUND)
    before = L.q4_handoff_timeouts()
    rec = observed.setdefault("hostile_vs_restatement", {}).setdefault(_key(geom, trait), {})
    t = q4.Transformer(hostile[geom, trait])
    try:
        for level in _levels(q4, geom):
            for graphs in (1, 0, 2):
                L.q4_set_fusion(level)
                L.q4_set_use_graphs(graphs)
                got, rows = _forced(q4, t)
                q4.check(L.q4_handoff_status(t.state))
                assert L.q4_get_fusion() == level and L.q4_handoff_timeouts() == before, (level, graphs)
                what = "level %d graphs %d" % (level, graphs)
                assert np.isfinite(got.astype(np.float32)).all(), what
                e = _rel(got, ref)
                rec["logits"] = max(rec.get("logits", 0.0), float(e.max()))
                assert e.max() <= bound, "%s: pos %d max rel logit err %g" % (what, int(e.max(axis=1).argmax()), e.max())
                for layer in range(t.config.n_layers):
                    for j in range(2):
                        gk, gv = rows[layer][j]
                        assert np.isfinite(gk.astype(np.float32)).all() and np.isfinite(gv.astype(np.float32)).all(), (what, layer, j)
                        ek, ev = float(_rel(gk, rk[layer, j]).max()), float(_rel(gv, rv[layer, j]).max())
                        rec["kv"] = max(rec.get("kv", 0.0), ek, ev)
                        assert ek <= kv_bound and ev <= kv_bound, (what, layer, j, ek, ev)
                # b. the unrounded double forward: 2x (+1e-3) on the maximum, 1.5x (+1e-4) on the rms over the vocabulary, as tests/test_baseline_configs_gpu.py
                for pos in range(F64_POSITIONS):
                    eg, er = float(_rel(got[pos], f64[pos]).max()), float(_rel(ref[pos], f64[pos]).max())
                    rg, rr = _rms(got[pos], f64[pos]), _rms(ref[pos], f64[pos])
                    rec["f64_max_gpu"] = max(rec.get("f64_max_gpu", 0.0), eg)
                    rec["f64_max_restatement"] = max(rec.get("f64_max_restatement", 0.0), er)
                    assert eg <= 2.0 * er + 1e-3, "%s pos %d: GPU %g vs restatement %g from the unrounded forward" % (what, pos, eg, er)
                    assert rg <= 1.5 * rr + 1e-4, "%s pos %d: rms GPU %g vs restatement %g from the unrounded forward" % (what, pos, rg, rr)
    finally:
        L.q4_set_fusion(q4.DEFAULT_FUSION)
        L.q4_set_use_graphs(1)
        t.close()


def _greedy(q4, t, level, steps, checkpoints, prompt):
    L = q4.lib()
    L.q4_set_fusion(level)
    t.reset(prompt)
    got = []
    for pos in range(steps):
        t.run_transformer(pos >= len(prompt) - 1)
        if pos in checkpoints:
            q4.synchronize()
            got.append(t.logits().view(np.uint16).copy())
    q4.synchronize()
    q4.check(L.q4_handoff_status(t.state))
    kv = np.stack([np.concatenate(t.kv_row(layer, p)) for layer in range(t.config.n_layers) for p in checkpoints]).view(np.uint16).copy()
    return got, [int(t.token(i)) for i in range(steps + 1)], kv


GREEDY = [(g, t) for g in ("ffn_pair7b", "head128") for t in hm.TRAITS]
STEPS = {"ffn_pair7b": (140, (3, 60, 127, 128, 139)), "head128": (600, (3, 100, 127, 128, 255, 256, 300, 511, 512, 599))}


@pytest.mark.parametrize("geom,trait", GREEDY)
def test_hostile_level_equalities(q4, hostile, observed, geom, trait):
    L = q4.lib()
    steps, checkpoints = STEPS[geom]
    prompt = [1, 5, 9]
    before = L.q4_handoff_timeouts()
    outs = {}
    t = q4.Transformer(hostile[geom, trait])
    try:
        for level in [3, 1, 0] + [lv for lv in _levels(q4, geom) if lv in (4, 5, 6)]:
            outs[level] = _greedy(q4, t, level, steps, checkpoints, prompt)
            assert L.q4_get_fusion() == level and L.q4_handoff_timeouts() == before, level
    finally:
        L.q4_set_fusion(q4.DEFAULT_FUSION)
        t.close()
    for level in (4, 5, 6):
        if level in outs:
            assert outs[level][1] == outs[3][1], "greedy token rings differ (level %d vs 3)" % level
            for a, b, pos in zip(outs[level][0], outs[3][0], checkpoints):
                assert np.array_equal(a, b), "logits differ at position %d (level %d vs 3)" % (pos, level)
            assert np.array_equal(outs[level][2], outs[3][2]), "K / V rows differ (level %d vs 3)" % level
    # level 0 vs 1: the same kernels, bit for bit (K = dim = 2560 / 4096: no shared half slot)
    assert outs[0][1] == outs[1][1], "token ring differs at fusion level 0"
    for a, b, pos in zip(outs[0][0], outs[1][0], checkpoints):
        assert np.array_equal(a, b), "logits differ at position %d (fusion 0 vs 1)" % pos
    # level 3 vs 1: another fp32 grouping inside the fused attention role -- the model's bound, equal rings until a near-tie
    first_div = next((i for i, (x, y) in enumerate(zip(outs[1][1], outs[3][1])) if x != y), None)
    rec = observed.setdefault("hostile_fusion3_vs_1", {}).setdefault(_key(geom, trait), {})
    rec["first_token_divergence"] = first_div
    min_div = FIRST_DIVERGENCE.get(_key(geom, trait), 128)
    assert first_div is None or first_div >= min_div, "token rings diverged at %d (fusion 3 vs 1)" % first_div
    # the benign rule of tests/test_forward_gpu.py; a model with its own bound against the restatement: twice that (both levels lie within it)
    own = BOUND.get(_key(geom, trait))
    for a, b, pos in zip(outs[1][0], outs[3][0], checkpoints):
        if first_div is not None and pos >= first_div:
            break
        err = float(_rel(a.view(np.float16), b.view(np.float16)).max())
        rec[str(pos)] = err
        assert err <= (2 * own if own else 5e-3 if pos <= 128 else 1.2e-2), (pos, err)
