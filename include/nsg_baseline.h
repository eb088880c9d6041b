/*
 * nsg_baseline.h -- C ABI of the fixed-block baseline coders of `libnsgcoder.so`: the Huffman coder of
 * code_base/huffman_baseline.py (with code_base/huffman.py) and the bins coder of code_base/block_baseline.py,
 * batched over B streams.  They work on the objects of nsg_coder.h: the same ns_ctx, ns_stream_state rows (only
 * bit_pos, ntokens and flags are used), [B, ld] logits rows (fp32 or fp16), LSB-first payload and output bits, the
 * HOST banned list, the sentence-end table of ns_set_sentence_end and the rank export of ns_set_rank_export.
 * Nothing allocates or synchronises; every call is stream-ordered and capturable.  One workgroup of one wave serves
 * one stream.
 *
 * block_size is 1..8 and K = 2^block_size must not exceed the ids left after the ban (NS_ERR_CONFIG otherwise).
 * There is no temperature, top-k or precision.
 *
 * Canonical definition (tests/baseline_cases.py restates it in Python):
 *   ranking   (value desc, id asc) on x + 0.0f, banned ids after every other id;
 *   Huffman   the K leaders get p_i = (float)(exp_canon(x_i - m) / S), m the top value, S the canonical full-row sum
 *             (oracle or_row_sum); the code tree is built by the operation sequence of CPython's heapq exactly as
 *             huffman.py drives it: heappush of leaves 0..K-1 in index order, then pop, pop, push of the merged node
 *             with the fp32 sum of the two weights, `<` on the weight alone, left = first popped; bit 0 goes left;
 *   bins      a device uint8[vocab] table gives every id's bin; bin v's token is the first id of the ranking inside
 *             the bin; the block's value is the LSB-first integer of its block_size bits.
 *   errors    a row with a NaN or +inf at an id that is not banned, a -inf among the K leaders (Huffman), or a bin
 *             whose first id is -inf or banned (bins) is NS_ST_ERR_RANGE | NS_ST_DONE: state and bits unchanged,
 *             nothing exported.
 *
 * Statistics: d_stats is an optional DEVICE [B][4] array of doubles in the layout of ns_set_stats, accumulated by
 * every message-phase encode step: [0] log p(selected) under the full softmax, [1] KL in bits of q against p --
 * Huffman: q_i = exp(-len_i * 0.69315) over the K leaders (huffman_baseline.py:55-58); bins: q = exp(-block_size *
 * 0.69315) at every bin's token (block_baseline.py:59-83), both divided by 0.69315 as code_base/utils.py:32-35 does
 * -- [2] untouched, [3] steps.  Float64 values; the reference's are fp32.
 *
 * NS_STEP_FINISH_SENT: a stream whose payload is consumed emits the canonical top-1 token per step until a
 * sentence-ending one (then NS_ST_DONE), as ns_encode_step does; without the flag it is NS_ST_DONE once
 * bit_pos >= nbits.  Encode reads a bit past the payload's end as 0, so bit_pos may end beyond nbits.
 *
 * d_trace, when given: k = kprime = K, sel = selected rank (Huffman) or bin (bins), n = bits consumed / emitted,
 * token, exact = 1, S = the row sum (0 where the step needs none: bins without statistics, sentence finishing).
 */
#ifndef NSG_BASELINE_H
#define NSG_BASELINE_H

#include "nsg_coder.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One Huffman encode step (huffman_baseline.py:24-65): the payload bits from bit_pos on walk the code tree from the
 * root to a leaf; the leaf's rank selects the token.  Arguments as ns_encode_step. */
int ns_huffman_encode_step(ns_ctx* ctx, const void* d_logits, int64_t ld, int B, int block_size,
                           const uint8_t* d_payload, int64_t payload_stride, const int64_t* d_payload_nbits,
                           ns_stream_state* d_state, int32_t* d_out_token, int32_t* d_token_hist, int64_t hist_stride,
                           const int32_t* banned, int nbanned, double* d_stats, ns_step_trace* d_trace,
                           uint32_t step_flags, void* hip_stream);

/* One Huffman decode step (huffman_baseline.py:93-163): the code of the received token's rank is appended LSB-first
 * to d_out_bits [B, out_stride] at bit_pos.  d_active: optional [B] mask.  A token that is not one of the K leaders
 * (a lower rank, a banned id, an id outside [0, vocab)) follows the divergence contract of ns_set_rank_export: state
 * and bits untouched, flags |= NS_ST_ERR_DIVERGE | NS_ST_DONE, and while an export is registered the K ranked ids go
 * to d_ranked[b*stride + i], i < min(K, stride), then -1 at index K when K < stride.  A code that does not fit the
 * out row is NS_ST_ERR_RANGE | NS_ST_DONE with nothing written (a row of 32 bytes per token always fits). */
int ns_huffman_decode_step(ns_ctx* ctx, const void* d_logits, int64_t ld, int B, int block_size,
                           const int32_t* d_in_token, const uint8_t* d_active, ns_stream_state* d_state,
                           uint8_t* d_out_bits, int64_t out_stride, const int32_t* banned, int nbanned,
                           ns_step_trace* d_trace, uint32_t step_flags, void* hip_stream);

/* The same step with each stream's token read from a DEVICE table at the stream's own ntokens, as
 * ns_decode_step_streams does: token t = ntokens from d_tokens[b*tok_stride + t]; parked at ntokens >= d_length[b]
 * or NS_ST_DONE; after a successful step the new bit_pos goes to d_counts[b*counts_stride + t] and the token to
 * d_out_token[b].  No host read is needed between steps. */
int ns_huffman_decode_step_streams(ns_ctx* ctx, const void* d_logits, int64_t ld, int B, int block_size,
                                   const int32_t* d_tokens, int64_t tok_stride, const int32_t* d_length,
                                   ns_stream_state* d_state, uint8_t* d_out_bits, int64_t out_stride,
                                   int64_t* d_counts, int64_t counts_stride, int32_t* d_out_token,
                                   const int32_t* banned, int nbanned, ns_step_trace* d_trace, uint32_t step_flags,
                                   void* hip_stream);

/* One bins encode step (block_baseline.py:43-91): the next block_size payload bits (LSB-first, a short tail padded
 * with zeros) name a bin of d_word2bin (DEVICE uint8[vocab], values < 2^block_size); the bin's token is emitted and
 * bit_pos advances by block_size. */
int ns_bins_encode_step(ns_ctx* ctx, const void* d_logits, int64_t ld, int B, int block_size,
                        const uint8_t* d_word2bin, const uint8_t* d_payload, int64_t payload_stride,
                        const int64_t* d_payload_nbits, ns_stream_state* d_state, int32_t* d_out_token,
                        int32_t* d_token_hist, int64_t hist_stride, const int32_t* banned, int nbanned,
                        double* d_stats, ns_step_trace* d_trace, uint32_t step_flags, void* hip_stream);

/* One bins decode step (block_baseline.py:119-187): block_size bits, the received token's bin LSB-first, when the
 * token is its bin's token.  Otherwise (an id outside [0, vocab) included) the stream diverges as above and the
 * export holds every bin's token in bin order: 2^block_size ids, then -1 when the stride leaves room. */
int ns_bins_decode_step(ns_ctx* ctx, const void* d_logits, int64_t ld, int B, int block_size,
                        const uint8_t* d_word2bin, const int32_t* d_in_token, const uint8_t* d_active,
                        ns_stream_state* d_state, uint8_t* d_out_bits, int64_t out_stride, const int32_t* banned,
                        int nbanned, ns_step_trace* d_trace, uint32_t step_flags, void* hip_stream);

int ns_bins_decode_step_streams(ns_ctx* ctx, const void* d_logits, int64_t ld, int B, int block_size,
                                const uint8_t* d_word2bin, const int32_t* d_tokens, int64_t tok_stride,
                                const int32_t* d_length, ns_stream_state* d_state, uint8_t* d_out_bits,
                                int64_t out_stride, int64_t* d_counts, int64_t counts_stride, int32_t* d_out_token,
                                const int32_t* banned, int nbanned, ns_step_trace* d_trace, uint32_t step_flags,
                                void* hip_stream);

#ifdef __cplusplus
}
#endif

#endif /* NSG_BASELINE_H */
