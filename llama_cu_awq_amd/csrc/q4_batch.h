// q4_batch.h -- batched decoding (q4_batch.hip): up to Q4_BATCH_MAX_SLOTS sequences over ONE Transformer's weights, every open one
// advanced by one position per pass over the weights. A slot owns what a sequence owns -- an fp16 K / V cache [n_layers][seq_len][kv_dim] x 2, a token ring,
// a position, a coin stream (its seed), a logits row -- and a pass runs the open slots as the rows of the pass layer loop (prompt_pass.h): row r is the slot
// map.slot[r] at that slot's position, rotated by that position, its K / V row written into that slot's cache, its attention over that cache alone. What a
// row computes is, bit for bit, what the per-token step computes at that position of that sequence (prompt_pass.hip's argument: a column's value is fixed by
// the staging, the chain over its k-slots and the epilogue; an attention block reads one row's q and one sequence's rows), so a slot's tokens, K / V rows
// and logits are those of the same checkpoint running that sequence alone -- whatever the other rows of the pass are.
// Not part of the C ABI; include/llama2_q4.h declares q4_batch_*.
#pragma once
#include "prompt_pass.h"

struct q4_snapshot;

namespace q4 {

constexpr int BATCH_MAX_SLOTS = PROMPT_PASS_MAX;
static_assert(BATCH_MAX_SLOTS == Q4_BATCH_MAX_SLOTS, "the public bound on a batch's slots is the pass's row count");

// The rows of one pass, by value in the embedding and pick launches' arguments: row r is slot[r]; coin[r] that slot's coin for this position
struct BatchRowMap { int n; int slot[BATCH_MAX_SLOTS]; float coin[BATCH_MAX_SLOTS]; };

// q4_snapshot.hip: what q4_batch_restore reads of a snapshot -- the packed rows (device; K rows [layer][n_pos][kv_dim], then V rows) and the tokens [n_pos]
const void* snapshot_rows(const q4_snapshot* s);
const int* snapshot_token_ids(const q4_snapshot* s);

}  // namespace q4
