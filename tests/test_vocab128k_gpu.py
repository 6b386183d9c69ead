"""Llama-3's vocabulary (128256) on the classifier side, on `cls128k`: cls4096's one-layer body (grouped-query 4:1) with a 128256 x 4096 classifier. The
strips launch at (4096, 128256) against the oracle's fp16 GEMV, the network in lockstep with the restatement from a prompt whose embedding rows lie beyond
2^29 bytes, the greedy step's int8 screen against the same model with the switch off, and the screen's op at d = 128256. The checkpoint is 2.1 GB: written
once per module, deleted behind it."""
import json
import os
import shutil
import tempfile

import numpy as np
import pytest

import cls_screen_ref as ref
from conftest import assert_close_f16
from llama_cu_awq_amd import synth
from test_baseline_configs_gpu import _lockstep

pytestmark = pytest.mark.gpu

N, D = 4096, 128256
SEED = 4242
X_SEED = SEED + N + 8           # the input vector whose float64 argmax over this matrix is row 99448 (margin 0.33): beyond 16 bits and beyond 98304
PROMPT = [1, 70001, 128255, 65536, 100003]                        # embedding rows at byte offsets 5.7e8 .. 1.05e9
GEN_PROMPT = PROMPT + [101, 13, 250, 77, 9, 410]                  # tests/test_cls_screen_gpu.py's prompt length: eight-step groups and a lone last step
STEPS = 40
# tests/test_gqa7b_gpu.py section a's bound: the restatement sits 4.9e-3 from the double forward on these 12 positions (profiles/gqa7b_parity_observed.json,
# cls128k / lockstep / vs_f64_restatement_max). The double forward costs 0.1 s of CPU per position at this vocabulary (measured: 0.49 s for five), so all
# 12 positions take the bracket
BOUND = 5e-3


@pytest.fixture(scope="module")
def model():
    d = tempfile.mkdtemp(prefix="cls128k")
    try:
        p = os.path.join(d, "cls128k.bin")
        synth.write_model(p, "cls128k", seed=31)
        yield p
    finally:
        shutil.rmtree(d, ignore_errors=True)


@pytest.fixture(scope="module")
def matrix(q4, model):
    """the op tests' classifier matrix and its device copy, made once, never modified: the checkpoint's own wcls (N(0, 0.02) as tests/test_ops_gpu.py's and
    cls_screen_ref.base_matrix's, row 2 zero), read back from the file -- drawing another 5e8 normals would take as long as everything else here"""
    w = np.fromfile(model, dtype=np.float16, count=D * N, offset=32 + 2 * D * N).reshape(D, N)
    dw = q4.DevBuf(w)
    yield w, dw
    dw.free()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float16).view(np.uint16)


def test_matmul_f16_at_the_llama3_classifier(q4, orc, rng, matrix):
    """the strips launch at (4096, 128256) -- 501 rows per CU at 256 CUs, a matrix of 1.05e9 bytes -- as tests/test_ops_gpu.py::test_matmul_f16"""
    w, dw = matrix
    x = rng.standard_normal(N).astype(np.float16)
    r16 = orc.matmul_f16(x, w.reshape(-1), N, D)
    r64 = ref.logits64(w, x)
    dx, do = q4.DevBuf(x), q4.DevBuf(nbytes=D * 2)
    q4.matmul(do, dx, dw, N, D)
    q4.synchronize()
    assert_close_f16(do.get(np.float16, D), r16, r64, what="fp16 gemv %dx%d" % (N, D))


def test_lockstep_with_the_restatement(q4, orc, model, observed):
    """Twelve positions (five prompt tokens with ids up to 128255, seven greedy tokens out of 128256) against the restatement and inside the bracket around
    the unrounded double forward at every position (tests/test_baseline_configs_gpu.py's _lockstep)."""
    t = q4.Transformer(model)
    m = orc.Model(model)
    try:
        rec = observed.setdefault("cls128k", {}).setdefault("lockstep", {})
        worst, compared, ties = _lockstep(q4, t, m, PROMPT, 12, 12, bound_vs_restatement=BOUND, rec=rec)
        print("cls128k lockstep: worst %.3e, %d tokens compared, %d near-ties" % (worst, compared, ties))
        assert compared == 8 and ties <= 2
        ring = [int(t.token(i)) for i in range(13)]
        rec["greedy_tokens"] = ring[len(PROMPT):]
        assert max(ring[len(PROMPT):]) >= 65536, ring                # (the restatement's greedy tokens do reach beyond 16 bits)
    finally:
        t.close()
        m.close()


def _run(q4, path, screen, graphs):
    L = q4.lib()
    L.q4_set_greedy_screen(int(screen))
    L.q4_set_use_graphs(graphs)
    try:
        t = q4.Transformer(path)
        toks = t.generate_ids(GEN_PROMPT, STEPS)[0].copy()
        logits = t.logits().copy()
        stats = t.screen_candidates()
        t.close()
    finally:
        L.q4_set_greedy_screen(1)
        L.q4_set_use_graphs(1)
    return toks, logits, stats


@pytest.mark.parametrize("graphs", [1, 2])
def test_generation_is_the_same_with_and_without_the_screen(q4, model, graphs):
    """tests/test_cls_screen_gpu.py's generation test at 128256 rows: the same tokens and final logits, bit for bit; every generating step but the last screened"""
    on_t, on_l, on_s = _run(q4, model, True, graphs)
    off_t, off_l, off_s = _run(q4, model, False, graphs)
    print(json.dumps({"geometry": "cls128k", "graphs": graphs, "last": on_s[0], "max": on_s[1], "total": on_s[2], "steps": on_s[3],
                      "tokens": [int(v) for v in on_t[len(GEN_PROMPT):]]}))
    assert np.array_equal(on_t, off_t)
    assert np.array_equal(_bits(on_l), _bits(off_l)), "the final position's logits differ"
    assert np.isfinite(on_l.astype(np.float32)).sum() > 0.9 * on_l.size, "the last step of the generation was screened"
    assert on_s[3] == STEPS - len(GEN_PROMPT) and on_s[1] >= on_s[0] >= 1 and on_s[2] >= on_s[1]
    assert off_s == (0, 0, 0, 0)
    assert int(on_t[len(GEN_PROMPT):].max()) >= 65536, on_t           # (greedy tokens beyond 16 bits did occur)


def _quantise_rows(w):
    """cls_screen_ref.quantise, a block of rows at a time (the matrix is 1 GB; the restatement's float32 temporaries would be four of it)"""
    parts = [ref.quantise(w[a:a + 8192]) for a in range(0, w.shape[0], 8192)]
    return tuple(np.concatenate([p[i] for p in parts]) for i in range(4))


def _screen_rows(quant, xs):
    q, s, E, W = quant
    parts = [ref.screen(q[a:a + 8192], s[a:a + 8192], E[a:a + 8192], W[a:a + 8192], xs) for a in range(0, q.shape[0], 8192)]
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


@pytest.fixture(scope="module")
def quantised(matrix):
    return _quantise_rows(matrix[0])


@pytest.mark.parametrize("name", ref.BENIGN + ("all rows identical",))
def test_screen_op_at_the_llama3_classifier(q4, matrix, quantised, observed, name):
    """tests/test_cls_screen_gpu.py::test_screen_op at n = 4096, d = 128256, its assertions: the bound on every row, the restated radius, the token by the
    lowest-index rule, refined entries -inf or the classifier's bits, at most 2 % candidates on the benign cases (the restatement alone: recorded below)."""
    base, dbase = matrix
    w, x, g = ref.make_case("benign" if name == "all rows identical" else name, base, N, X_SEED, D)
    dw, quant = dbase, quantised
    if name == "all rows identical":                                 # row 0 of the base matrix, 128256 times (make_case would copy the gigabyte to say so)
        w = np.repeat(base[:1], D, axis=0)
        dw = q4.DevBuf(w)
        one = ref.quantise(w[:8])
        quant = tuple(np.repeat(a[:1], D, axis=0) for a in one)
    dx, dg = q4.DevBuf(x), (q4.DevBuf(g) if g is not None else None)
    dxs = dx
    if dg is not None:
        dxs = q4.DevBuf(nbytes=2 * N)
        q4.rmsnorm(dxs, dx, dg, N)
    dl = q4.DevBuf(nbytes=2 * D)
    q4.matmul(dl, dxs, dw, N, D)
    q4.synchronize()
    L = dl.get(np.float16, D)
    xs = dxs.get(np.float16, N)
    token, A, B, refined, cand = q4.greedy_screen_op(dx, dw, N, D, dg)
    if dw is not dbase:
        dw.free()

    Lf = L.astype(np.float64)
    claim = np.isfinite(B)
    with np.errstate(invalid="ignore"):
        ratio = np.abs(A[claim].astype(np.float64) - Lf[claim]) / B[claim].astype(np.float64)
    rA, rB = _screen_rows(quant, xs)
    both = claim & np.isfinite(rB)
    # the restatement's own candidates (tests/test_cls_screen_host.py's rule): rows whose interval reaches the best lower end, and rows without a claim
    rclaim = np.isfinite(rB)
    restated = int(((rA + rB >= (rA - rB)[rclaim].max()) | ~rclaim).sum())
    rec = {"case": name, "n": N, "d": D, "candidates": cand, "restatement_candidates": restated, "restatement_share": restated / D,
           "rows_without_claim": int((~claim).sum()), "max_err_over_B": float(ratio.max()) if ratio.size else None, "token": token}
    print(json.dumps(rec))
    observed.setdefault("cls128k", {}).setdefault("screen_op", {})[name] = rec
    assert np.isfinite(A[claim]).all() and np.isfinite(Lf[claim]).all(), "a finite radius beside a non-finite value"
    assert (ratio <= 1.0).all(), "%s: |A - L| > B on %d rows, worst ratio %g" % (name, int((ratio > 1.0).sum()), ratio.max())
    assert (B[both] >= rB[both] * (1 - 1e-5)).all() and (B[both] <= rB[both] * (1 + 4e-3) + 1e-7).all()
    assert (np.abs(A[both] - rA[both]) <= 0.01 * rB[both]).all(), "A is not the restatement's s (q . x)"
    want = ref.argmax_lowest(L)
    assert token == want, "%s: token %d, argmax of the full logits %d" % (name, token, want)
    rb, lb = _bits(refined), _bits(L)
    kept = rb != 0xFC00
    assert (rb[kept] == lb[kept]).all(), "%s: %d refined entries are neither -inf nor L's bits" % (name, int((rb[kept] != lb[kept]).sum()))
    assert (rb[~claim] == lb[~claim]).all(), "a row without a claim was not refined"
    with np.errstate(invalid="ignore"):
        tied = L.astype(np.float32) == L.astype(np.float32)[want]
    assert (rb[tied] == lb[tied]).all() and rb[want] == lb[want]
    assert int(kept.sum()) <= cand <= int(kept.sum()) + int((lb == 0xFC00).sum())
    if name in ref.BENIGN:
        assert restated <= 0.02 * D, "the restatement alone: %d of %d rows" % (restated, D)
        assert cand <= 0.02 * D, "%s: %d of %d rows are candidates" % (name, cand, D)
        assert want > 98304, want                                    # (on the reference's logits: X_SEED)
    if name == "all rows identical":
        assert cand == D and token == 0
