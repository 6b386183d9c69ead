// q4_batch.h -- batched decoding (q4_batch.hip): up to Q4_BATCH_MAX_SLOTS sequences over ONE Transformer's weights, every open one
// advanced by one position per pass over the weights. A slot owns what a sequence owns -- an fp16 K / V cache [n_layers][seq_len][kv_dim] x 2, a token ring,
// a position, a coin stream (its seed), a logits row -- and a pass runs the open slots as the rows of the pass layer loop (prompt_pass.h): row r is the slot
// map.slot[r] at that slot's position, rotated by that position, its K / V row written into that slot's cache, its attention over that cache alone. What a
// row computes is, bit for bit, what the per-token step computes at that position of that sequence (prompt_pass.hip's argument: a column's value is fixed by
// the staging, the chain over its k-slots and the epilogue; an attention block reads one row's q and one sequence's rows), so a slot's tokens, K / V rows
// and logits are those of the same checkpoint running that sequence alone -- whatever the other rows of the pass are.
// With q4_batch_set_prefill above 1 a slot inside its prompt takes several rows of a pass, consecutive positions (q4_batch_plan_rows): the argument above
// is per row, so which pass carries a position changes no byte of it.
// Not part of the C ABI; include/llama2_q4.h declares q4_batch_*.
#pragma once
#include "prompt_pass.h"

struct q4_snapshot;

namespace q4 {

constexpr int BATCH_MAX_SLOTS = PROMPT_PASS_MAX;
static_assert(BATCH_MAX_SLOTS == Q4_BATCH_MAX_SLOTS, "the public bound on a batch's slots is the pass's row count");

// The rows of one pass, by value in the embedding, gather and pick launches' arguments. Row r is slot[r] at that slot's position + off[r]: a slot's rows
// are adjacent, ascending and consecutive, slots in slot order (q4_batch_plan_rows). The m slots of the pass, in that order, are its "last rows": last[j]
// is the row that carries slot j-of-the-pass's highest position -- the only row whose token or logits anyone needs --, cnt[j] that slot's row count (what
// its position advances by), coin[j] its coin for that highest position. One row per slot (the default): m = n, last[j] = j, off = 0, cnt = 1.
struct BatchRowMap {
    int n, m;
    int slot[BATCH_MAX_SLOTS], off[BATCH_MAX_SLOTS];
    int last[BATCH_MAX_SLOTS], cnt[BATCH_MAX_SLOTS];
    float coin[BATCH_MAX_SLOTS];
};

// q4_snapshot.hip: what q4_batch_restore reads of a snapshot -- the packed rows (device; K rows [layer][n_pos][kv_dim], then V rows) and the tokens [n_pos]
const void* snapshot_rows(const q4_snapshot* s);
const int* snapshot_token_ids(const q4_snapshot* s);

}  // namespace q4
