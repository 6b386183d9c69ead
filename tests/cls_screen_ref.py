"""float64 restatement of the greedy screen's quantiser and bound (csrc/cls_screen.h), and the op-level cases shared by the GPU and the host tests.

Row r of the fp16 matrix w, as real numbers: s = max|w| / 127 (float32), q = clip(rint(w / s), -127, 127), e = w - s q, E = ||e||_2,
W = max(||w||_2, s ||q||_2). For a staged fp16 input x: A = s (q . x), X = ||x||_2 and
    B = (E + GAMMA W) X (1 + 2^-11) + 2^-11 |A| + 2^-24
bounds |A - L| for L the fp16 logit of the classifier (an fp32 sum of at most 28 roundings rounded once to fp16), whatever the order of the sums."""
import numpy as np

GAMMA = 64 * 2.0 ** -23          # csrc/cls_screen.h: 28 fp32 roundings on the classifier's longest path + 36 on the screen's, 2^-23 each
F16_MAX = 65504.0


def quantise(w16):
    """(q int8 [d, n], s float32 [d], E float64 [d], W float64 [d]); a row with an inf or a NaN gets s = 0, q = 0, E = inf."""
    w = np.asarray(w16, dtype=np.float16).astype(np.float32)
    finite = np.isfinite(w).all(axis=1)
    w = np.where(finite[:, None], w, np.float32(0))
    s = (np.abs(w).max(axis=1) / np.float32(127)).astype(np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(s[:, None] > 0, np.rint(w / s[:, None]), np.float32(0))
    q = np.clip(q, -127, 127)
    d = w.shape[0]
    E, W = np.empty(d), np.empty(d)
    for a in range(0, d, 2048):                                 # float64 a block of rows at a time
        wb, qb, sb = w[a:a + 2048].astype(np.float64), q[a:a + 2048].astype(np.float64), s[a:a + 2048].astype(np.float64)
        e = wb - sb[:, None] * qb
        E[a:a + 2048] = np.sqrt((e * e).sum(axis=1))
        W[a:a + 2048] = np.maximum(np.sqrt((wb * wb).sum(axis=1)), sb * np.sqrt((qb * qb).sum(axis=1)))
    E[~finite] = np.inf
    return q.astype(np.int8), s, E, W


def screen(q, s, E, W, x16):
    """(A, B) float64 of the restatement for the staged input x16; B = inf where |A| + B reaches fp16's overflow range or is NaN"""
    x = np.asarray(x16, dtype=np.float16).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        A = s.astype(np.float64) * (q.astype(np.float64) @ x) if np.isfinite(x).all() else np.full(q.shape[0], np.nan)
        X = np.sqrt((x * x).sum())
        B = (E + GAMMA * W) * X * (1 + 2.0 ** -11) + 2.0 ** -11 * np.abs(A) + 2.0 ** -24
        B = np.where(np.abs(A) + B < F16_MAX, B, np.inf)
    return A, B


def logits64(w16, x16):
    """w . x in float64, row blocks"""
    x = np.asarray(x16, dtype=np.float16).astype(np.float64)
    out = np.empty(w16.shape[0])
    with np.errstate(invalid="ignore", over="ignore"):
        for a in range(0, w16.shape[0], 2048):
            out[a:a + 2048] = w16[a:a + 2048].astype(np.float64) @ x
    return out


def rmsnorm16(x16, w16):
    """the staged input behind the final norm (rmsnorm_kernel's arithmetic up to the order of the fp32 sum): half(x * (ss * w))"""
    x = np.asarray(x16, dtype=np.float16).astype(np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        ss = np.float32(1.0) / np.sqrt(np.float32((x.astype(np.float64) ** 2).sum() / x.shape[0]) + np.float32(1e-5))
        return (x * (ss * np.asarray(w16, dtype=np.float16).astype(np.float32))).astype(np.float16)


def argmax_lowest(l16):
    """argmax_kernel's rule: the largest value, the lowest index among ties; 0 when nothing compares greater than -inf (all -inf / NaN)"""
    v = np.asarray(l16, dtype=np.float16).astype(np.float32)
    v = np.where(np.isnan(v), -np.inf, v)
    m = v.max()
    return 0 if m == -np.inf else int(np.argmax(v == m))


def base_matrix(n, d, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((d, n), dtype=np.float32) * np.float32(0.02)).astype(np.float16)


def input_vector(n, seed, spikes=False):
    rng = np.random.default_rng(seed + 7)
    x = rng.standard_normal(n).astype(np.float32)
    if spikes:
        at = rng.choice(n, size=8, replace=False)
        x[at] = np.where(rng.random(8) < 0.5, -300.0, 300.0)
    return x.astype(np.float16)


def norm_weight(n, seed):
    return (1.0 + 0.1 * np.random.default_rng(seed + 11).uniform(-1, 1, n)).astype(np.float16)


# name -> (changes the matrix?, benign?). Every case runs behind the final norm (raw x, norm weight) except "benign, x as it is".
CASES = ("benign", "benign, x as it is", "all-zero row", "two identical rows, both the maximum", "all rows identical", "scales over three decades",
         "a row of +-65504", "x with eight channels at +-300", "x containing a NaN", "x = 0")
BENIGN = ("benign", "benign, x as it is")


def make_case(name, base, n, seed, d=None):
    """(w16 or None for the base matrix, raw x16, norm weight or None). `base` is base_matrix(n, rows >= d, seed): never modified; the case lives in
    its first d rows (rows behind them only pad the matrix for a reference that wants a multiple of eight)."""
    d = base.shape[0] if d is None else d
    rng = np.random.default_rng(seed + 23)
    x, g, w = input_vector(n, seed), norm_weight(n, seed), None
    if name == "benign, x as it is":
        x, g = rmsnorm16(x, g), None
    elif name == "all-zero row":
        w = base.copy()
        w[[2, d // 2, d - 1]] = 0
    elif name == "two identical rows, both the maximum":
        xs = rmsnorm16(x, g).astype(np.float32)
        w = base.copy()
        row = (np.sign(xs) * 0.02).astype(np.float16)           # far above every N(0, 0.02) row's logit
        w[d - 5] = row
        w[d // 3] = row
    elif name == "all rows identical":
        w = np.repeat(base[:1], base.shape[0], axis=0)
    elif name == "scales over three decades":
        w = (base.astype(np.float32) * (10.0 ** rng.uniform(-1.5, 1.5, base.shape[0])).astype(np.float32)[:, None]).astype(np.float16)
    elif name == "a row of +-65504":
        xs = rmsnorm16(x, g).astype(np.float32)
        w = base.copy()
        w[d // 2] = np.where(xs >= 0, F16_MAX, -F16_MAX).astype(np.float16)     # +inf as an fp16 logit
        w[d // 2 + 17] = np.where(xs >= 0, -F16_MAX, F16_MAX).astype(np.float16)   # -inf
    elif name == "x with eight channels at +-300":
        x = input_vector(n, seed, spikes=True)
    elif name == "x containing a NaN":
        x = x.copy()
        x[n // 3] = np.nan
    elif name == "x = 0":
        x = np.zeros(n, dtype=np.float16)
    elif name != "benign":
        raise KeyError(name)
    return w, x, g
