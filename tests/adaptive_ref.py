"""numpy restatement of the adaptive truncation launch (csrc/q4_adaptive.hip; the rule is in include/llama2_q4.h): top-n-sigma, typical-p and
Mirostat v2 over fp16 logits. Elementwise operations are float32 where the rule says fp32 (v = float(l), w = v / t, the parameters themselves);
every SUM is float64: the kernel's sums have a fixed order numpy cannot follow, so its thresholds are held to these within a tolerance, and its masks
are then recomputed EXACTLY, in float32, from the thresholds it recorded (expect_from_record).
Also here, because tests and tools/measure_adaptive_parity.py share them: the op-level test inputs and the deviation of a record from this file."""
import numpy as np

F = np.float32
D = np.float64
NEUTRAL = dict(typical_p=1.0, top_n_sigma=0.0, mirostat_tau=0.0, mirostat_eta=0.1)
LOG2E, LN2 = D(F(1.44269504088896340736)), D(F(0.69314718055994530942))       # the kernel's fp32 constants
FIELDS = ("T_s", "H", "d_star", "mu", "T_m", "kept", "lse", "lse_t")
NEG_INF_BITS = 0xFC00


def controls(**kw):
    c = dict(NEUTRAL)
    c.update(kw)
    return {k: D(F(v)) for k, v in c.items()}                  # the launch sees float32 values


def lse64(a):
    a = np.asarray(a, dtype=D)
    m = a.max()
    return D(m + np.log(np.exp(a - m).sum()))


class Chain:
    """Mirostat's state: mu by position, the side buffer of the last launch"""

    def __init__(self):
        self.mu = {}
        self.side = None
        self.side_pos = -1
        self.side_lse = D("nan")


def typical_tiers(v64, part):
    """(lse, s, H, d, tier values ascending, cumulative mass per tier) of the entries that take part, float64"""
    lse = lse64(v64[part])
    s = lse - v64
    p = np.where(part, np.exp(-np.where(part, s, 0.0)), 0.0)
    H = D((p[part] * s[part]).sum())
    d = np.abs(s - H)
    tiers, inv = np.unique(d[part], return_inverse=True)
    cum = np.cumsum(np.bincount(inv, weights=p[part], minlength=tiers.shape[0]))
    return lse, s, H, d, tiers, cum


def run(x16, c, temperature=1.0, chain=None, pos=0, tok=None):
    """the rule in float64 sums: (logits after the launch as float16, record dict of float64 -- NaN where a stage was off --, extras for the checks)"""
    c = controls(**c)
    x = np.asarray(x16, dtype=np.float16)
    out = x.copy()
    v = x.astype(F)
    part = np.isfinite(v)
    rec = {k: D("nan") for k in FIELDS}
    extra = {}
    if c["top_n_sigma"] > 0 and part.any():
        vv = v[part].astype(D)
        m, mean = vv.max(), vv.sum() / vv.shape[0]
        sigma = np.sqrt(((vv - mean) ** 2).sum() / vv.shape[0])
        rec["T_s"] = m - c["top_n_sigma"] * sigma
        extra["sigma"] = sigma
        part = part & (v.astype(D) >= rec["T_s"])
    if c["typical_p"] < 1 and part.any():
        lse, s, H, d, tiers, cum = typical_tiers(v.astype(D), part)
        at = int(np.searchsorted(cum, c["typical_p"], side="left"))       # the first tier whose cumulative mass reaches typical_p
        at = min(at, tiers.shape[0] - 1)                                   # none does: everything stays
        rec["lse"], rec["H"], rec["d_star"] = lse, H, tiers[at]
        extra["tiers"], extra["cum"] = tiers, cum
        part = part & (d <= tiers[at])
    if c["mirostat_tau"] > 0 and chain is not None:
        t = F(temperature)
        with np.errstate(invalid="ignore"):
            w = (v / t).astype(D)                                          # ONE fp32 division, as the rule says
        prev = chain.mu.get(pos - 1, D("nan")) if pos > 0 else D("nan")
        if np.isnan(prev):
            mu = 2.0 * c["mirostat_tau"]
        elif chain.side_pos == pos - 1 and tok is not None and 0 <= tok < x.shape[0] and np.isfinite(chain.side[tok]):
            surprise = (chain.side_lse - chain.side[tok]) * LOG2E
            mu = prev - c["mirostat_eta"] * (surprise - c["mirostat_tau"])
        else:
            mu = prev
        rec["mu"] = mu
        chain.mu[pos] = mu
        chain.side_pos = -1
        if part.any():
            wm = w[part].max()
            rec["lse_t"] = lse64(w[part])
            rec["T_m"] = rec["lse_t"] - mu * LN2
            keep = part & (w >= rec["T_m"])
            keep[int(np.nonzero(part & (w == wm))[0][0])] = True
            part = keep
            chain.side = np.where(part, w, -np.inf)
            chain.side_lse = lse64(w[part])
            chain.side_pos = pos
    out[np.isfinite(v) & ~part] = -np.inf
    rec["kept"] = int(part.sum())
    return out, rec, extra


def expect_from_record(x16, rec, temperature=1.0):
    """the logits behind the launch, EXACTLY: every mask recomputed in float32 from the thresholds (and lse, H) the launch recorded. Returns
    (float16 logits, the float32 deviations d_i of stage 2 or None, the entries that took part in stage 2 or None)"""
    x = np.asarray(x16, dtype=np.float16)
    v = x.astype(F)
    part = np.isfinite(v)
    d, part2 = None, None
    with np.errstate(invalid="ignore"):
        if not np.isnan(rec["T_s"]):
            part = part & (v >= F(rec["T_s"]))
        if not np.isnan(rec["d_star"]):
            part2 = part.copy()
            s = F(rec["lse"]) - v
            d = np.abs(s - F(rec["H"]))
            part = part & (d <= F(rec["d_star"]))
        if not np.isnan(rec["T_m"]):
            w = v / F(temperature)
            wm = w[part].max()
            keep = part & (w >= F(rec["T_m"]))
            keep[int(np.nonzero(part & (w == wm))[0][0])] = True
            part = keep
    out = x.copy()
    out[np.isfinite(v) & ~part] = -np.inf
    return out, d, part2


# ---------------------------------------------------------------------------------------------------------------------------------
# what the op-level tests and the parity measurement share
# (32779: the looping form with tail elements; 128256 / 128259: Llama-3's vocabulary and one with tail elements -- sixteen loop runs, ids beyond 16 bits)
SIZES = (1, 7, 64, 1000, 8192, 32768, 32776, 32000, 32779, 128256, 128259)
HIGH = 65536                     # a size above it: the entries below this id lie 40 under the others, so the maximum, its ties and whatever a stage keeps sit at ids >= HIGH
# (name, controls, temperature): every stage alone, typical-p at two masses, everything together (top-n-sigma wide enough to leave a distribution)
CONFIGS = (
    ("top-n-sigma 1", dict(top_n_sigma=1.0), 1.0),
    ("typical-p 0.9", dict(typical_p=0.9), 1.0),
    ("typical-p 0.5", dict(typical_p=0.5), 1.0),
    ("Mirostat 5 at 0.8", dict(mirostat_tau=5.0, mirostat_eta=0.1), 0.8),
    ("all three", dict(top_n_sigma=2.5, typical_p=0.9, mirostat_tau=3.0, mirostat_eta=0.2), 0.8),
)


def inputs(n):
    """(name, float16 logits): seeded normal logits at scales 1 and 8, a one-hot (+30 over zeros), all equal, 10 % -inf and one NaN, two values only
    (every deviation is one of two: the ties sit at the boundary)"""
    rng = np.random.default_rng(9100 + n)
    out = [("normal x1", rng.standard_normal(n).astype(np.float16)), ("normal x8", (rng.standard_normal(n) * 8.0).astype(np.float16))]
    lo = HIGH if n > HIGH else 0
    hot = np.zeros(n, dtype=np.float16)
    hot[100003 if lo else n // 3] = 30.0
    out.append(("one-hot", hot))
    out.append(("all equal", np.full(n, -1.25, dtype=np.float16)))
    holes = (rng.standard_normal(n) * 2.0).astype(np.float16)
    holes[rng.random(n) < 0.1] = -np.inf
    holes[n // 2] = np.nan
    out.append(("-inf and NaN", holes))
    two = np.where(rng.random(n) < 0.25, 2.0, 0.5).astype(np.float16)
    out.append(("two values", two))
    for _, x in out:
        x[:lo] = (x[:lo].astype(F) - F(40.0)).astype(np.float16)
    return out


def mass_eps(x16):
    """how far the fp32 mass of a kept set may lie from float64: every p_i = expf(-(lse - v_i)) carries lse's error (the log-probability bound
    2^-24 * (2 |l - m| + 3 ln n + 64), at most once more for the subtraction and expf's 2 ulp), and the sum of at most n terms of total <= 1 in runs of
    32 plus two trees adds 2^-24 * 64: twice the log-probability bound at the FARTHEST entry covers both"""
    x = np.asarray(x16).astype(D)
    f = x[np.isfinite(x)]
    if f.size == 0:
        return 0.0
    return 2.0 * 2.0 ** -24 * (2.0 * (f.max() - f.min()) + 3.0 * np.log(x.shape[0]) + 64.0)


def lse_bound(a64):
    """q4_logprobs' bound for lse itself: 2^-24 * (3 ln n + 64)"""
    return 2.0 ** -24 * (3.0 * np.log(max(np.asarray(a64).shape[0], 1)) + 64.0)


def deviations(x16, got, want, extra, c):
    """per measured quantity, |kernel - float64| / max(1, |float64|) of one launch's record `got` against run()'s `want`: T_s, H, d_star. d_star is
    measured against the INTERVAL of tiers float64 admits -- the first tier whose cumulative mass reaches typical_p - eps up to the first that reaches
    typical_p + eps (eps = mass_eps): a mass within rounding of typical_p at a tier boundary may fall on either side."""
    out = {}
    for k in ("T_s", "H"):
        if not np.isnan(want[k]):
            out[k] = abs(D(got[k]) - want[k]) / max(1.0, abs(want[k]))
    if not np.isnan(want["d_star"]):
        tiers, cum = extra["tiers"], extra["cum"]
        tp, eps = controls(**c)["typical_p"], mass_eps(x16)
        lo = tiers[min(int(np.searchsorted(cum, tp - eps, side="left")), tiers.shape[0] - 1)]
        hi = tiers[min(int(np.searchsorted(cum, tp + eps, side="left")), tiers.shape[0] - 1)]
        g = D(got["d_star"])
        out["d_star"] = max(lo - g, g - hi, 0.0) / max(1.0, abs(want["d_star"]))
    return out


def mu_tolerance(tol_prev, eta, tau, side_lse, side_tok, mu):
    """|fp32 mu - float64 mu| after one update mu = prev - eta * ((side_lse - side_tok) * log2e - tau): prev's own tolerance, the side log-sum-exp's
    bound scaled by eta * log2e, and half an ulp (2^-24 relative) of each of the four fp32 results"""
    diff = abs(side_lse - side_tok)
    surprise = diff * LOG2E
    over = abs(surprise - tau)
    return tol_prev + eta * LOG2E * (lse_bound(np.zeros(32000)) + 2.0 ** -24 * diff) + 2.0 ** -24 * (eta * (surprise + over) + eta * over + abs(mu))


def staged(x16, got, c, temperature=1.0, chain=None, pos=0, tok=None, mu_tol=0.0):
    """One launch's record `got` (dict of FIELDS) against this file, stage by stage: each stage's float64 statistics are taken over what the launch's OWN
    recorded thresholds left of the stages in front (so a boundary entry that rounding puts on the other side does not leak into the next stage's
    reference). Returns (the float16 logits the launch must have left -- exact --, deviations {T_s, H, d_star} as deviations() defines them,
    bounded [(name, got, want, tolerance)] for lse, lse_t, mu, T_m, minimality (kept mass, kept mass without the outermost tier, eps) or None)"""
    cc = controls(**c)
    nan = {k: D("nan") for k in FIELDS}
    cur = np.asarray(x16, dtype=np.float16)
    dev, bounded, minimal = {}, [], None
    if cc["top_n_sigma"] > 0:
        _, want, extra = run(cur, dict(top_n_sigma=c["top_n_sigma"]))
        dev.update(deviations(cur, got, want, extra, dict(top_n_sigma=c["top_n_sigma"])))
        cur = expect_from_record(cur, dict(nan, T_s=got["T_s"]))[0]
    if cc["typical_p"] < 1:
        sub = dict(typical_p=c["typical_p"])
        _, want, extra = run(cur, sub)
        if not np.isnan(want["lse"]):
            v64 = cur.astype(D)
            bounded.append(("lse", D(got["lse"]), want["lse"], lse_bound(v64)))
            dev.update(deviations(cur, got, want, extra, sub))
            nxt, d32, part2 = expect_from_record(cur, dict(nan, lse=got["lse"], H=got["H"], d_star=got["d_star"]))
            kept = part2 & np.isfinite(nxt.astype(F))
            p64 = np.where(part2, np.exp(-(want["lse"] - np.where(part2, v64, 0.0))), 0.0)
            if kept.any():                                     # (an empty kept set fails the exact comparison: no need to fail here)
                outer = kept & (d32 == d32[kept].max())
                minimal = (D(p64[kept].sum()), D(p64[kept & ~outer].sum()), mass_eps(cur))
            cur = nxt
    if cc["mirostat_tau"] > 0 and chain is not None:
        _, want, _ = run(cur, dict(mirostat_tau=c["mirostat_tau"], mirostat_eta=c["mirostat_eta"]), temperature, chain, pos, tok)
        bounded.append(("mu", D(got["mu"]), want["mu"], mu_tol + 2.0 ** -24 * abs(want["mu"])))
        if not np.isnan(want["lse_t"]):
            lt = lse_bound(cur.astype(D))
            bounded.append(("lse_t", D(got["lse_t"]), want["lse_t"], lt))
            tm = lt + LN2 * (mu_tol + 2.0 ** -24 * abs(want["mu"])) + 2.0 ** -23 * (abs(want["lse_t"]) + abs(want["mu"] * LN2))
            bounded.append(("T_m", D(got["T_m"]), want["T_m"], tm))
            cur = expect_from_record(cur, dict(nan, T_m=got["T_m"]), temperature)[0]
    return cur, dev, bounded, minimal
