"""Which branch of topp_sample_kernel (csrc/q4_sampling.hip) an input takes, restated in numpy from the kernel's own conditions, and the crafted
inputs that populate every branch: distributions with holes -- a few, a few hundred or a few thousand finite logits, -inf everywhere else -- which is
what top-k, typical-p, top-n-sigma and a guide leave the sampler.

The label is INFERRED from restated probabilities (numpy's float32 exp, a float64 sum), not observed on the device: an input whose mass sits within
rounding of a branch condition may be labelled one branch off. Nothing asserts on a label but the census (tests/test_sampler_paths_host.py), which is a
condition on the inputs; token parity (tests/test_sampler_paths_gpu.py) does not depend on it.

Labels. The form comes first: `pre` (softmax_spread_kernel + topp_sample_kernel<true>: n <= 32768, n % 8 == 0, T > 0), `one-block`
(topp_sample_kernel<false>, n <= 32768), `global` (n > 32768: the passes through global memory, no shortcut -- its softmax returns no top entry). Then
    top-alone                    the largest probability alone reaches the threshold
    scan/vector, scan/scalar     topp outside (0, 1): no sort; E == 32 and n % 8 == 0 reads its keys with 16-byte loads
    lists<nb>/wave0 | /block     pre only: nb exponent-band lists taken, m <= 1024 candidates scanned by wave 0 (ceil(m / E) <= 64) or by the block
    <why>cut9 | cut11 | cut12    radix-sorted candidates at the cut 2^-9 / 2^-11 / 2^-12 (whether or not their scan then hits: a miss goes on to the full
                                 sort and cannot be told from outside)
    <why>too-many                the chosen cut holds more than 4096 candidates: full sort
    <why>none                    no cut's mass covers the threshold: full sort
<why>, pre only, says why the lists were not scanned: `overflow/` (a band above 1024 entries), `wide/` (m > 1024), `short/` (the four lists' mass does
not cover `need`). A `lists` label also stands for "lists scanned, missed, fell through": one label per entry, as for the cuts."""
import numpy as np

F = np.float32
NINF = float("-inf")
T_THREADS, MAX_E = 1024, 32

# the vocabulary sizes both test modules run: E = ceil(n / 1024) is 1, 1, 1, 1, 2, 8, 16, 17, 20, 32, 32, 32, 33, 40, 126, 126 (Llama-3's vocabulary and
# one that is no multiple of eight: the global-memory form's loops run four times, and token ids pass 16 bits)
SIZES = (64, 1000, 1001, 1024, 2048, 8192, 16384, 16392, 20000, 32000, 32003, 32768, 32776, 40000, 128256, 128259)
HIGH = 65536                                                     # a size above it: every finite logit sits at an id >= HIGH, so every token that can be drawn does
SUPPORTS = (1, 2, 3, 40, 64, 65, 500, 1000, 1024, 1025, 1500, 2048, 2049, 3000, 4096, 4097, 6000)      # ... and n itself
SETTINGS = ((0.8, 0.9), (0.5, 0.6), (1.0, 1.0))                  # (temperature, topp)
TIED = (1030, 2050, 4100)                                        # equal entries that straddle a band's 1024, a cut's 2048 and its 4096
MIN_TRIALS = 110


def probs(x16, T):
    """the fp16 probabilities orc_sample_topp computes: half(l / T), fp32 expf, rounded to half, divided by the fp32 sum of the unrounded
    exponentials, rounded to half. (numpy's exp and a float64 sum stand in for expf and the kernel's tree: good enough to classify.)"""
    x = np.asarray(x16, dtype=np.float16).astype(F)
    with np.errstate(over="ignore", invalid="ignore"):
        v = (x / F(T)).astype(np.float16).astype(F)
        e = np.exp(v - v.max()).astype(F)
        total = F(e.astype(np.float64).sum())
        return (e.astype(np.float16).astype(F) / total).astype(np.float16)


def form(n, T):
    if n > T_THREADS * MAX_E:
        return "global"
    return "pre" if n % 8 == 0 and T > 0 else "one-block"


def _cut(p32, bits, need):
    """the radix-candidate path: the smallest of {p >= 2^-9}, {>= 2^-11}, {>= 2^-12} whose mass covers `need`, at most 4096 entries"""
    for name, ex in (("cut9", 6), ("cut11", 4), ("cut12", 3)):
        sel = bits >= (ex << 10)
        if F(p32[sel].astype(np.float64).sum()) >= need:
            return "too-many" if int(sel.sum()) > 4096 else name
    return "none"


def classify(x16, n, T, topp, coin):
    """the name of the branch topp_sample_kernel takes for logits x16[:n], the sampler's (T, topp) and this coin"""
    do_sort = not (topp <= 0 or topp >= 1)
    threshold = F(coin) * F(topp) if do_sort else F(coin)
    f = form(n, T)
    E = (n + T_THREADS - 1) // T_THREADS
    if not do_sort:
        if f == "global":
            return "global/scan"
        return f + ("/scan/vector" if E == MAX_E and n % 8 == 0 else "/scan/scalar")
    if f == "global":
        return "global/sort"
    p = probs(np.asarray(x16)[:n], T)
    bits, p32 = p.view(np.uint16), p.astype(F)
    if p32.max() >= threshold:
        return f + "/top-alone"
    need = F(threshold * F(1.01) + F(0.004))
    why = ""
    if f == "pre":
        ex = (bits >> 10).astype(np.int64)
        cand = bits >= (3 << 10)                                 # fp16 bits of 2^-12: exponent field 3
        band = np.where(ex >= 6, 0, 6 - ex)
        count = [int((cand & (band == b)).sum()) for b in range(4)]
        if max(count) > T_THREADS:
            why = "overflow/"
        else:
            mass = [F(p32[cand & (band == b)].astype(np.float64).sum()) for b in range(4)]
            nb, run = 0, F(0)
            for b in range(4):
                run = F(run + mass[b])
                if run >= need:
                    nb = b + 1
                    break
            m = sum(count[:nb])
            if 0 < m <= T_THREADS:
                return "pre/lists%d/%s" % (nb, "wave0" if (m + E - 1) // E <= 64 else "block")
            why = "wide/" if m > T_THREADS else "short/"
    return f + "/" + why + _cut(p32, bits, need)


def _fill(rng, kind, k):
    if kind == "equal":
        return np.full(k, float(np.float16(rng.standard_normal())))
    return rng.standard_normal(k) * (0.3 if kind == "x0.3" else 2.0)


def low_id(n):
    """the least id a finite logit has at this size"""
    return HIGH if n > HIGH else 0


def _holed(rng, n, k, values):
    x = np.full(n, NINF, dtype=np.float16)
    lo = low_id(n)
    x[lo + rng.choice(n - lo, size=k, replace=False)] = np.asarray(values, dtype=np.float16)
    return x


# Distributions laid out by exponent band and AIMED at one branch, for the branches that random supports and random coins reach seldom or never.
# `big` entries share what the rest leaves of the mass (each at least 2^-9: band 0); c1, c2, c3 entries lie in the bands [2^-10, 2^-9),
# [2^-11, 2^-10), [2^-12, 2^-11) at m1, m2, m3 times the band's lower edge; `tail` entries of 1.9 x 2^-13 lie below every band. With S0 = 0 and
# S1 .. S4 the cumulative masses of the bands, S5 = 1.01 topp + 0.004 (what `need` = threshold x 1.01 + 0.004 stays below), the window (lo, hi) asks for
# S_lo < need <= S_hi: (k - 1, k) takes k lists where no list overflows and at most 1024 candidates are taken, (4, 5) is "the four lists do not cover
# it"; in the one-block form and behind an overflow the same sums decide the cut. The trial then takes the seed's NEXT coin inside the range that puts
# `need` there (coin_range: the draws in between are discarded -- the stream is the seed's own, a few draws further on), so a branch that only two
# per cent of the thresholds lead to is fed like any other. classify() has the last word on the label: the census counts what it says.
# (name, big, (c1, c2, c3), (m1, m2, m3), tail, window, {vocabulary size: repeats})
_E1 = (1000, 1001, 1024)
_LARGE = (8192, 16384, 16392, 20000, 32000, 32003, 32768)
AIMED = (
    ("two lists of 64", 4, (60, 0, 0), (1.9, 0, 0), 0, (1, 2), {64: 10}),
    ("two lists of 60", 4, (56, 900, 0), (1.9, 1.5, 0), 0, (1, 2), {n: 10 for n in (1000, 1024)}),
    ("three lists of 60", 4, (4, 52, 900), (1.4, 1.9, 1.9), 0, (2, 3), {n: 10 for n in (1000, 1024)}),
    ("four lists of 64", 4, (2, 2, 56), (1.4, 1.4, 1.9), 900, (3, 4), {n: 10 for n in (1000, 1024)}),
    ("four lists of 1000 within 1000", 100, (12, 12, 876), (1.4, 1.4, 1.9), 0, (3, 4), {n: 10 for n in _E1}),
    ("two lists of 600", 20, (580, 0, 0), (1.4, 0, 0), 0, (1, 2), {n: 10 for n in (1000, 1024, 2048)}),
    ("three lists of 870", 10, (60, 800, 0), (1.4, 1.9, 0), 0, (2, 3), {n: 10 for n in (1000, 1024, 2048)}),
    ("tail of 900", 8, (0, 0, 0), (0, 0, 0), 900, (4, 5), {n: 10 if n <= 2048 else 4 for n in _E1 + (2048,) + _LARGE}),
    ("one list of 300", 300, (0, 0, 0), (0, 0, 0), 0, (0, 1), {2048: 10}),
    ("two lists of 110", 10, (100, 0, 0), (1.9, 0, 0), 1800, (1, 2), {2048: 10}),
    ("three lists of 118", 4, (4, 110, 1000), (1.4, 1.9, 1.9), 800, (2, 3), {2048: 10}),
    ("four lists of 118", 4, (4, 4, 110), (1.4, 1.4, 1.9), 1900, (3, 4), {2048: 10}),
    ("four lists of 1000 within 2048", 10, (36, 54, 900), (1.4, 1.9, 1.9), 860, (3, 4), {2048: 10}),
    ("1304 in three lists", 4, (300, 1000, 0), (1.05, 1.3, 0), 0, (2, 3), {2048: 10}),
    ("1100 in four lists", 10, (36, 54, 1000), (1.4, 1.9, 1.9), 860, (3, 4), {2048: 10}),
    ("band 3 of 1300 behind 50: the large ones cover", 50, (0, 0, 1300), (0, 0, 1.9), 0, (0, 1), {2048: 10}),
    ("band 3 of 1300 behind 50", 50, (0, 0, 1300), (0, 0, 1.9), 0, (3, 4), {2048: 10}),
    ("band 2 of 1100 behind 10", 10, (0, 1100, 0), (0, 1.1, 0), 0, (2, 3), {2048: 10}),
    ("band 3 of 1030 over a tail", 6, (0, 0, 1030), (0, 0, 1.05), 1000, (4, 5), {2048: 10}),
    ("two lists of 620", 20, (600, 0, 0), (1.4, 0, 0), 0, (1, 2), {8192: 9}),
    ("two lists of 420", 20, (400, 0, 0), (1.9, 0, 0), 0, (1, 2), {n: 9 for n in _LARGE}),
    ("three lists of 880", 10, (70, 800, 0), (1.4, 1.9, 0), 0, (2, 3), {8192: 9}),
    ("three lists of 500", 10, (40, 450, 0), (1.4, 1.9, 0), 2000, (2, 3), {n: 9 for n in _LARGE}),
    ("four lists of 1000", 10, (36, 54, 900), (1.4, 1.9, 1.9), 1900, (3, 4), {8192: 9}),
    ("four lists of 490", 5, (15, 20, 450), (1.4, 1.9, 1.9), 3100, (3, 4), {n: 9 for n in _LARGE}),
    ("1205 in three lists", 5, (200, 1000, 0), (1.05, 1.05, 0), 1100, (2, 3), {n: 9 for n in _LARGE}),
    ("1155 in four lists", 5, (50, 100, 1000), (1.05, 1.05, 1.5), 2200, (3, 4), {n: 9 for n in _LARGE}),
    ("band 3 of 1100 behind 200: the large ones cover", 200, (0, 0, 1100), (0, 0, 1.1), 1000, (0, 1), {n: 9 for n in _LARGE}),
    ("band 3 of 1100", 2, (0, 0, 1100), (0, 0, 1.1), 3000, (3, 4), {n: 9 for n in _LARGE}),
    ("band 3 of 1100: no cut covers", 2, (0, 0, 1100), (0, 0, 1.1), 3000, (4, 5), {n: 9 for n in _LARGE}),
    ("band 2 of 1100 behind 10 over a tail", 10, (0, 1100, 0), (0, 1.1, 0), 1000, (2, 3), {n: 9 for n in _LARGE}),
)
TAIL_P = 1.9 * 2.0 ** -13
MARGIN = 0.006                                                   # of `need` from the window's ends: the fp16 roundings move a mass by a few 1e-3


def _aimed(rng, n, T, topp, big, counts, mults, tail, window):
    """(float16 logits [n] whose softmax at temperature T has the layout, the coin range that puts `need` inside the window)"""
    groups = [mults[b] * 2.0 ** -(10 + b) * (1.0 + 0.01 * rng.uniform(-1, 1, counts[b])) for b in range(3)] + [np.full(tail, TAIL_P)]
    rest = 1.0 - sum(g.sum() for g in groups)
    p_big = rest / big
    assert p_big >= 1.05 * 2.0 ** -9 and big + sum(counts) + tail <= n, "the layout does not fit"
    S = [0.0, rest]
    for g in groups[:3]:
        S.append(S[-1] + g.sum())
    S.append(1.01 * topp + 0.004)
    lo, hi = S[window[0]], min(S[window[1]], S[5])
    margin = min(MARGIN, (hi - lo) / 4.0)
    c_lo, c_hi = (lo + margin - 0.004) / 1.01 / topp, (hi - margin - 0.004) / 1.01 / topp
    c_lo = max(c_lo, 1.02 * p_big / topp, 0.0)                   # (above the largest probability: no top-alone shortcut)
    if not c_lo < c_hi <= 1.0:                                   # (no coin leads there at this topp: the caller takes the other setting)
        return None, None
    p = np.concatenate([np.full(big, p_big)] + groups)
    return _holed(rng, n, p.shape[0], T * np.log(p / p.max())), (c_lo, c_hi)


ANY_COIN = (0.0, 1.0)


def next_coin(random_f32, state, coin_range):
    """the seed's stream up to its next coin inside coin_range: (the state in front of that draw -- what a Sampler must hold to draw it --, the coin)"""
    import ctypes as C
    while True:
        before = state.value
        coin = random_f32(C.byref(state))
        if coin_range[0] <= coin < coin_range[1]:
            return before, coin


def cases(n, round_=0):
    """[(name, float16 logits [n], T, topp, coin range)]: every support size k <= n at seeded random indices, -inf elsewhere, filled with equal
    values, normal x 0.3 and normal x 2, each at the three settings; tied supports that straddle a band's 1024, a cut's 2048 and its 4096; one dense
    normal vector with 10 % holes. No all -inf vector and no NaN: the restatement's own softmax is NaN there."""
    rng = np.random.default_rng(1000003 * round_ + n)
    out = []

    def add(name, x):
        for T, topp in SETTINGS:
            out.append(("%s, T %g topp %g" % (name, T, topp), x, T, topp, ANY_COIN))

    lo = low_id(n)
    for k in sorted(set(s for s in SUPPORTS if s <= n - lo) | {n - lo}):
        for kind in ("equal", "x0.3", "x2"):
            add("support %d %s" % (k, kind), _holed(rng, n, k, _fill(rng, kind, k)))
    for k in TIED:
        if k <= n - lo:
            add("%d tied" % k, _holed(rng, n, k, np.zeros(k)))
    x = (rng.standard_normal(n) * 2.0).astype(np.float16)
    x[rng.random(n) < 0.1] = NINF
    x[:lo] = NINF
    if not np.isfinite(x.astype(F)).any():
        x[lo] = 0.0
    add("dense normal x2, 10 % holes", x)
    return out


def aimed_cases(n):
    """the AIMED layouts of this size at the two sorted settings in turn, and 4097 equal entries"""
    rng = np.random.default_rng(7000003 + n)
    out = []
    for name, big, counts, mults, tail, window, repeats in AIMED:
        for rep in range(repeats.get(n, 0)):
            T, topp = SETTINGS[rep % 2]
            x, coin_range = _aimed(rng, n, T, topp, big, counts, mults, tail, window)
            if x is None:
                T, topp = SETTINGS[1 - rep % 2]
                x, coin_range = _aimed(rng, n, T, topp, big, counts, mults, tail, window)
            assert x is not None, name + ": no coin leads there"
            out.append(("%s #%d, T %g topp %g" % (name, rep, T, topp), x, T, topp, coin_range))
    if 4097 + 4 <= n <= T_THREADS * MAX_E:
        # 4097 equal entries: 1 / 4097 lies half an fp16 ulp under 2^-12 and rounds UP to it (ties to even), so 4097 candidates pass the cut
        # 2^-12 -- the one way past its cap of 4096. A few entries 14 below (e^-14/T of the sum: the rounding stands) make other inputs of it
        for extra in range(0, 5):
            v = np.concatenate([np.zeros(4097), np.full(extra, -14.0)])
            for T, topp in SETTINGS[:2]:
                out.append(("4097 equal and %d far below, T %g topp %g" % (extra, T, topp), _holed(rng, n, 4097 + extra, v), T, topp, (0.01, 1.0)))
    return out


def trials(n):
    """the cases of as many rounds (other seeds) as it takes to reach MIN_TRIALS, then the aimed ones"""
    out, r = [], 0
    while len(out) < MIN_TRIALS:
        out += cases(n, r)
        r += 1
    return out + aimed_cases(n)


# No prefix reaches the threshold: k equal entries whose fp16 probabilities, rounded down one by one, add up to an fp16 total below a coin of
# 0.9999 (FALLBACK_STATE is the xorshift state, 5765 draws behind seed 1, whose next coin is 0.999900281). The search then falls back to the
# order's last entry with a probability above 0, which for equal entries is also the textbook answer -- the cumulative mass passes 0.9999 at the last
# of them -- while index n - 1, here a -inf logit, is not. (size, topp, support sizes): the unsorted scan and the sorted one in every form.
FALLBACK_STATE = 11221404413583269187
FALLBACK = (
    (1001, 1.0, (6, 11, 14)), (1001, 0.99999, (109, 119, 191)),
    (2048, 1.0, (6, 7, 10)), (2048, 0.99999, (218, 238, 382)),
    (32000, 1.0, (6, 7, 11)), (32000, 0.99999, (6, 7, 11)),
    (32776, 1.0, (6, 7, 10)), (32776, 0.99999, (6, 7, 11)),
)


def fallback_case(n, k):
    """(float16 logits [n] with k entries of 0.5 among the first n - 1 and -inf elsewhere, the last of the k indices)"""
    rng = np.random.default_rng(k)
    x = np.full(n, NINF, dtype=np.float16)
    idx = np.sort(rng.choice(n - 1, size=k, replace=False))
    x[idx] = 0.5
    return x, int(idx[-1])
