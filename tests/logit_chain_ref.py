"""The four logit stages of a generating step as ONE reference, in the order of csrc/q4_step.hip's STAGES table: the guide's mask (guide_ref), DRY
(dry_ref, with q4_dry_penalty_table's table), the sampling controls (sampling_controls_ref), the adaptive truncation (adaptive_ref). The first three
are bit-exact restatements. The adaptive stage follows tests/test_adaptive_gpu.py's contract and adds no tolerance of its own: the launch's recorded
thresholds are held to float64 within adaptive_ref.staged's bounds, and the mask is recomputed exactly, in float32, from the recorded thresholds."""
import numpy as np

import adaptive_ref
import dry_ref
import guide_ref
import sampling_controls_ref

F, D = np.float32, np.float64
ORDER = ("guide", "dry", "controls")                             # the exact stages, as STAGES has them; the adaptive stage is always last


def front(raw16, ring, pos, guide_table, guide_states, dry, pen, controls, bias, order=ORDER):
    """the three exact stages over the raw fp16 logits of position `pos`, in `order` (ORDER: the step's own; another one serves the test's check that
    the order can be told at all). guide_states: the reference's state ring, written at `pos`. dry / controls None: the stage is off.
    Returns float16 logits."""
    x = np.array(raw16, dtype=np.float16)
    for stage in order:
        if stage == "guide" and guide_table is not None:
            x = guide_ref.mask(x, guide_table, guide_states, ring, pos)[0].view(np.float16)
        elif stage == "dry" and dry is not None:
            x = dry_ref.apply(x, ring, pos, pen, **dry)[0]
        elif stage == "controls" and (controls is not None or bias):
            x = sampling_controls_ref.process(x, tokens=ring, pos=pos, logit_bias=bias, **(controls or {}))
    return x


def rebase(chain, discard):
    """q4_shift_context moved Mirostat's ring and the side buffer's position down by `discard`: the reference's chain follows"""
    chain.mu = {p - discard: m for p, m in chain.mu.items() if p - discard >= 0}
    if chain.side_pos >= 0:
        chain.side_pos -= discard


def chain(raw16, ring, pos, guide_table, guide_states, dry, pen, controls, bias, adaptive, adaptive_record, temperature, mirostat=None, mu_tol=0.0):
    """One generating step at `pos`. adaptive: the stage's settings or None; adaptive_record: the launch's own record at `pos` (dict of
    adaptive_ref.FIELDS); mirostat: the adaptive_ref.Chain of the run (None: Mirostat is off); mu_tol: the tolerance of mu the chain has accumulated.
    Returns (the float16 logits the sampler / argmax must have found, the logits behind the third stage, deviations, bounded, minimal, mu_tol):
    the last four as adaptive_ref.staged returns them, mu_tol advanced by this step's update."""
    x3 = front(raw16, ring, pos, guide_table, guide_states, dry, pen, controls, bias)
    if adaptive is None:
        return x3, x3, {}, [], None, mu_tol
    tok = int(ring[pos])
    if mirostat is not None and adaptive.get("mirostat_tau", 0) > 0 and pos > 0 and mirostat.side_pos == pos - 1 and not np.isnan(
            mirostat.mu.get(pos - 1, D("nan"))) and 0 <= tok < x3.shape[0] and np.isfinite(mirostat.side[tok]):
        mu_tol = adaptive_ref.mu_tolerance(mu_tol, adaptive["mirostat_eta"], adaptive["mirostat_tau"], mirostat.side_lse, mirostat.side[tok],
                                           mirostat.mu[pos - 1])
    out, dev, bounded, minimal = adaptive_ref.staged(x3, adaptive_record, adaptive, temperature, mirostat, pos, tok, mu_tol)
    if mirostat is not None and adaptive.get("mirostat_tau", 0) > 0 and mirostat.side_pos == pos:
        # the side buffer the NEXT update reads describes what the launch itself kept (its recorded threshold), not what float64 would have kept
        with np.errstate(invalid="ignore", divide="ignore"):
            w = (out.astype(F) / F(temperature)).astype(D)
        kept = np.isfinite(w)
        if kept.any():
            mirostat.side = np.where(kept, w, -np.inf)
            mirostat.side_lse = adaptive_ref.lse64(w[kept])
    return out, x3, dev, bounded, minimal, mu_tol
