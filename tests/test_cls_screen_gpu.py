"""The greedy step's classifier as an int8 screen + exact refinement (csrc/cls_screen.h): at the op level against q4_matmul_f16 and the float64
restatement of the bound (cls_screen_ref.py), and inside the token loop against the same model with the switch off.

Held at the op level, for EVERY row r: |A_r - L_r| <= B_r with L from q4_matmul_f16 on the same inputs (a row with B = +inf makes no claim: it must be
refined; d = 64 CUs + 77 is no multiple of eight, which q4_matmul_f16 wants: the reference runs over the matrix padded by three rows the op never
sees); the token is argmax L by the lowest-index rule; every refined entry is -inf or bit-equal to L_r; the entries at the argmax and at every row
tied with it are bit-equal. Benign inputs: at most 2 % of the rows are candidates (the restatement alone gives <= 0.81 % on these shapes)."""
import json
import os
import tempfile

import numpy as np
import pytest

import cls_screen_ref as ref
from llama_cu_awq_amd import synth

pytestmark = pytest.mark.gpu

SEED = 4242
PROMPT = [1, 20, 300, 7, 45, 101, 13, 250, 77, 9, 410]          # prompt steps, the prompt -> generate boundary, full eight-step groups, the lone last step
STEPS = 40


def _shapes(q4):
    cus = q4.device_info()[1]
    return {4096: 64 * cus + 77, 5120: 64 * cus}                # a ragged split over the blocks; the least the strips form admits


_SHARED = {}


def _base(q4, n):
    """per shape, computed once and left unchanged: the base matrix, its device copy, its restated quantisation"""
    if n not in _SHARED:
        d = _shapes(q4)[n]
        w = ref.base_matrix(n, (d + 7) // 8 * 8, SEED + n)      # q4_matmul_f16 takes multiples of eight rows: the reference runs over the padded matrix
        _SHARED[n] = (d, w, q4.DevBuf(w), ref.quantise(w[:d]))
    return _SHARED[n]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float16).view(np.uint16)


@pytest.mark.parametrize("name", ref.CASES)
@pytest.mark.parametrize("n", [4096, 5120])
def test_screen_op(q4, n, name):
    d, base, dbase, qbase = _base(q4, n)
    w, x, g = ref.make_case(name, base, n, SEED + n, d)
    dw = dbase if w is None else q4.DevBuf(w)
    quant = qbase if w is None else ref.quantise(w[:d])
    dpad = base.shape[0]
    dx, dg = q4.DevBuf(x), (q4.DevBuf(g) if g is not None else None)
    # the reference: q4_matmul_f16 on the same inputs (behind q4_rmsnorm where the case has a norm weight)
    dxs = dx
    if dg is not None:
        dxs = q4.DevBuf(nbytes=2 * n)
        q4.rmsnorm(dxs, dx, dg, n)
    dl = q4.DevBuf(nbytes=2 * dpad)
    q4.matmul(dl, dxs, dw, n, dpad)                             # (a row's logit does not depend on the rows behind it)
    q4.synchronize()
    L = dl.get(np.float16, d)
    xs = dxs.get(np.float16, n)
    token, A, B, refined, cand = q4.greedy_screen_op(dx, dw, n, d, dg)

    Lf = L.astype(np.float64)
    claim = np.isfinite(B)
    with np.errstate(invalid="ignore"):
        ratio = np.abs(A[claim].astype(np.float64) - Lf[claim]) / B[claim].astype(np.float64)
    rA, rB = ref.screen(*quant, xs)
    both = claim & np.isfinite(rB)
    print(json.dumps({"case": name, "n": n, "d": d, "candidates": cand, "rows_without_claim": int((~claim).sum()),
                      "max_err_over_B": float(ratio.max()) if ratio.size else None,
                      "median_B": float(np.median(B[claim])) if claim.any() else None,
                      "max_B_over_restated_B": float((B[both] / rB[both]).max()) if both.any() else None,
                      "min_B_over_restated_B": float((B[both] / rB[both]).min()) if both.any() else None}))
    # the bound, every row
    assert np.isfinite(A[claim]).all() and np.isfinite(Lf[claim]).all(), "a finite radius beside a non-finite value"
    assert (ratio <= 1.0).all(), "%s: |A - L| > B on %d rows, worst ratio %g" % (name, int((ratio > 1.0).sum()), ratio.max())
    # ... which is the restated one: never below it (the kernel inflates X by 2^-10 and B by 2^-20), and not blown up
    assert (B[both] >= rB[both] * (1 - 1e-5)).all() and (B[both] <= rB[both] * (1 + 4e-3) + 1e-7).all()
    assert (np.abs(A[both] - rA[both]) <= 0.01 * rB[both]).all(), "A is not the restatement's s (q . x)"
    # the token and the refined logits
    want = ref.argmax_lowest(L)
    assert token == want, "%s: token %d, argmax of the full logits %d" % (name, token, want)
    rb, lb = _bits(refined), _bits(L)
    kept = rb != 0xFC00
    assert (rb[kept] == lb[kept]).all(), "%s: %d refined entries are neither -inf nor L's bits" % (name, int((rb[kept] != lb[kept]).sum()))
    assert (rb[~claim] == lb[~claim]).all(), "a row without a claim was not refined"
    with np.errstate(invalid="ignore"):
        tied = L.astype(np.float32) == L.astype(np.float32)[want]
    assert (rb[tied] == lb[tied]).all() and rb[want] == lb[want]
    assert int(kept.sum()) <= cand <= int(kept.sum()) + int((lb == 0xFC00).sum())      # (a refined row whose logit IS -inf looks like a row left out)
    if name in ref.BENIGN:
        assert cand <= 0.02 * d, "%s: %d of %d rows are candidates" % (name, cand, d)
    if name in ("all rows identical", "x containing a NaN", "x = 0"):
        assert cand == d and token == 0


# ---------------------------------------------------------------------------------------------------------------------------------
# inside the token loop
@pytest.fixture(scope="module")
def model_dir():
    with tempfile.TemporaryDirectory() as d:
        yield d


def _path(model_dir, geometry):
    path = os.path.join(model_dir, geometry + ".bin")
    if not os.path.exists(path):
        synth.write_model(path, geometry, seed=31)
    return path


def _run(q4, path, screen, graphs, **kw):
    L = q4.lib()
    L.q4_set_greedy_screen(int(screen))
    L.q4_set_use_graphs(graphs)
    try:
        before = L.q4_graph_captures()
        t = q4.Transformer(path, **kw)
        toks = t.generate_ids(PROMPT, STEPS)[0].copy()
        logits = t.logits().copy()
        stats = t.screen_candidates()
        captures = L.q4_graph_captures() - before
        t.close()
    finally:
        L.q4_set_greedy_screen(1)
        L.q4_set_use_graphs(1)
    return toks, logits, stats, captures


@pytest.mark.parametrize("graphs", [1, 2])
@pytest.mark.parametrize("geometry", ["cls4096", "cls5120", "cls4096_ragged"])
def test_generation_is_the_same_with_and_without_the_screen(q4, model_dir, geometry, graphs):
    path = _path(model_dir, geometry)
    on_t, on_l, on_s, _ = _run(q4, path, True, graphs)
    off_t, off_l, off_s, _ = _run(q4, path, False, graphs)
    print(json.dumps({"geometry": geometry, "graphs": graphs, "last": on_s[0], "max": on_s[1], "total": on_s[2], "steps": on_s[3]}))
    assert np.array_equal(on_t, off_t)
    assert np.array_equal(_bits(on_l), _bits(off_l)), "the final position's logits differ"
    assert np.isfinite(on_l.astype(np.float32)).sum() > 0.9 * on_l.size, "the last step of the generation was screened"
    # every generating step but the last: positions len(PROMPT) - 1 .. STEPS - 2
    assert on_s[3] == STEPS - len(PROMPT) and on_s[1] >= on_s[0] >= 1 and on_s[2] >= on_s[1]
    assert off_s == (0, 0, 0, 0)


def test_sampled_steps_and_steps_with_records_are_not_screened(q4, model_dir):
    path = _path(model_dir, "cls4096_ragged")
    assert _run(q4, path, True, 1, temperature=0.5)[2][3] == 0
    assert _run(q4, path, True, 1, logprobs=0)[2][3] == 0


def test_a_model_without_a_copy_is_left_alone(q4, model_dir):
    path = _path(model_dir, "small")
    on_t, on_l, on_s, on_c = _run(q4, path, True, 1)
    off_t, off_l, off_s, off_c = _run(q4, path, False, 1)
    assert on_c == off_c and on_c > 0, "graph captures: %d with the switch on, %d with it off" % (on_c, off_c)
    assert on_s == (0, 0, 0, 0) and off_s == (0, 0, 0, 0)
    assert np.array_equal(on_t, off_t) and np.array_equal(_bits(on_l), _bits(off_l))
