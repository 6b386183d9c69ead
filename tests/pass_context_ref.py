"""Python restatement of where the token loop takes a prompt pass or a verify pass once q4_set_pass_context lets passes above position 255
(csrc/q4_passes.hip: pass_attention_plan, prompt_pass_tokens, verify_covers). Pure arithmetic on positions: no GPU, no library.

The rules restated:
  * a pass touches positions below min(bound, seq_len) only, bound = max(256, the value set);
  * a pass stays inside the bin of its first position: [0, 256), [256, 512), [512, 1024), [1024, 2048), ...;
  * at every position it touches, the step's attention form must be one the pass reproduces: the V-slice forms where the step's bin argument is at
    most 256, a split-context form where it is at least 512 (chunks of 64 / 128 / 256 positions for arguments up to 512 / 1024 / above) -- and one
    chunk size for the whole pass. The bin argument of the step at `pos` is the graph bin of pos + 1 with graphs (mode 1) and eager bins (mode 2), and
    pos + 1 itself without graphs (mode 0), where arguments 257 .. 511 give the one-block form: no pass."""
import numpy as np

T = 8                 # PROMPT_PASS_MAX
MAX_DRAFT = 7
MAX_GRAPHS = 8        # Q4_MAX_GRAPHS
SPLIT_MIN = 512       # the smallest bin argument that runs the split-context form (q4_set_attention_split's default)


def bin_end(pos):
    end = 256
    while end <= pos:
        end *= 2
    return end


def graph_bin(seq_len, model_seq_len):
    """graph_bin of q4_step.hip: 128, 256, ... for the first MAX_GRAPHS - 1 bins, the model's seq_len behind them"""
    b = 128
    for _ in range(MAX_GRAPHS - 1):
        if seq_len <= b:
            return b
        b *= 2
    return model_seq_len


def bin_arg(pos, mode, model_seq_len):
    return pos + 1 if mode == 0 else graph_bin(pos + 1, model_seq_len)


def form(pos, mode, model_seq_len):
    """'v' (V-slice), the chunk size of the split-context form, or None (a form no pass reproduces)"""
    arg = bin_arg(pos, mode, model_seq_len)
    if arg >= SPLIT_MIN:
        return 64 if arg <= 512 else 128 if arg <= 1024 else 256
    return "v" if arg <= 256 else None


def covers(pos, n, bound, model_seq_len, mode=1):
    """may one pass take positions pos .. pos + n - 1?"""
    limit = min(max(bound, 256), model_seq_len)
    if n < 1 or pos + n > limit or pos + n > bin_end(pos):
        return False
    kinds = {form(pos + i, mode, model_seq_len) for i in range(n)}
    return None not in kinds and len(kinds) == 1


def prompt_passes(n_prompt, steps, bound, model_seq_len, start=0, mode=1, ingest=T):
    """[(pos, n)] of the prompt passes of a generation: positions start .. n_prompt - 2 are prompt-only; a pass takes up to `ingest` of them, at least
    2. Wherever no pass is admitted the loop runs steps; a step group never reaches across a graph bin, and a position where a pass is refused for
    its length alone (one position left in front of a bin end, of the prompt's end or of `steps`) is stepped alone, so the next question is asked at
    pos + 1."""
    out = []
    pos = start
    last = min(n_prompt - 1, steps)
    while pos < last:
        n = min(last - pos, ingest, bin_end(pos) - pos, min(max(bound, 256), model_seq_len) - pos)
        if n >= 2 and covers(pos, n, bound, model_seq_len, mode):
            out.append((pos, n))
            pos += n
        else:
            pos += 1
    return out


def replay(run, n_prompt, steps, drafter, max_draft, group, bound, model_seq_len, mode=1):
    """tests/spec_ref.py's replay with the cuts above: at every generating position the drafter may draft up to the largest room <= max_draft for which
    positions pos .. pos + room lie inside `steps`, the bound and one bin with an admitted form. Returns ((passes, drafted, accepted), [(pos, n_draft,
    accepted)])."""
    run = [int(x) for x in run]
    passes = []
    pos = n_prompt - 1
    while pos < steps:
        room = min(max_draft, steps - 1 - pos)
        while room >= 1 and not covers(pos, room + 1, bound, model_seq_len, mode):
            room -= 1
        d = [int(x) for x in drafter(np.asarray(run[:pos + 1], dtype=np.int32), room)][:room] if room >= 1 else []
        if d:
            m = 0
            while m < len(d) and d[m] == run[pos + 1 + m]:
                m += 1
            passes.append((pos, len(d), m))
            pos += m + 1
        else:
            pos += group(pos)
    return (len(passes), sum(p[1] for p in passes), sum(p[2] for p in passes)), passes
