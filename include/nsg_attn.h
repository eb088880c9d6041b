/*
 * nsg_attn.h -- decode-step attention of the batched GPT-2 forward (row a19 of SURVEY.md §8), part of
 * `libnsgcoder.so`.
 *
 * Replaces, for one new token per stream, the attention of the reference's per-token forward
 * `model(prev, past_key_values=past, position_ids=...)` (code_base/arithmetic.py:115-122, the Hugging Face
 * GPT2Attention over the whole unbounded cache: softmax(q k^T / sqrt(D)) v).  It fuses the KV append of
 * the new token with the attention over the cache: one wavefront per (stream, head) streams the K and V rows
 * of that head once from HBM (online softmax in fp32), so the step is HBM-bound at B*(L+1)*2*D*2 bytes per
 * layer.  A pair's rows are split over 1, 2, 4 or 8 waves by the key count alone (one wave up to 256 keys, eight
 * beyond 1,024), partials merged in wave order: the summation order -- and every output bit -- does not depend on
 * the batch size, so the decoder of a cover reproduces the encoder's logits at any B.  fp16 in and out, fp32
 * accumulation; no allocation, stream-ordered on the caller's hipStream_t.
 */
#ifndef NSG_ATTN_H
#define NSG_ATTN_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* One layer, one decode position.
 *   d_qkv     fp16 [B, qkv_stride]: q at columns [0, H*D), k at [H*D, 2*H*D), v at [2*H*D, 3*H*D) (the c_attn
 *             output of GPT-2, head h at columns h*D..h*D+D-1 of each part).
 *   d_k_cache, d_v_cache  fp16, element (b, h, j, d) at b*cache_b_stride + h*cache_h_stride + j*D + d.
 *   L0        positions already cached; the call writes the new k/v at position L0 and attends to
 *             positions 0..L0 (L0 + 1 keys).  The caller guarantees L0 < the cache's capacity.
 *   d_out     fp16 [B, out_stride]: head h of stream b at columns h*D..h*D+D-1.
 *   scale     the score scale (1/sqrt(D) for GPT-2).
 * D must be 64.  Returns 0, or a negative NS_ERR_* code of nsg_coder.h on bad arguments / launch failure. */
int ns_decode_attention(const void* d_qkv, int64_t qkv_stride, void* d_k_cache, void* d_v_cache,
                        int64_t cache_b_stride, int64_t cache_h_stride, int B, int H, int D, int L0, void* d_out,
                        int64_t out_stride, float scale, void* hip_stream);

/* The same with the cache length read from device memory (*d_L0, int32) when the kernel runs, so one captured
 * hipGraph serves every decode step; `cap` = the cache capacity in positions (a step with *d_L0 >= cap writes
 * and reads nothing). */
int ns_decode_attention_dev(const void* d_qkv, int64_t qkv_stride, void* d_k_cache, void* d_v_cache,
                            int64_t cache_b_stride, int64_t cache_h_stride, int B, int H, int D, const int32_t* d_L0,
                            int cap, void* d_out, int64_t out_stride, float scale, void* hip_stream);

/* The general form: positions [0, T0) are a prefix SHARED by all B streams (the common context, stored once:
 * element (h, j, d) at h*prefix_h_stride + j*D + d, j < T0), positions [T0, L0] are the stream's own rows at
 * index r = j - T0 of d_k_cache / d_v_cache, grouped in 32-row chunks: element (b, h, r, d) at
 * b*cache_b_stride + h*cache_h_stride + (r/32)*cache_chunk_stride + (r%32)*D + d.  cache_chunk_stride = 0 (or
 * 32*D) is the plain per-pair row-contiguous layout; a chunk-plane layout (cache_chunk_stride = B*H*32*D,
 * cache_b_stride = H*32*D, cache_h_stride = 32*D) keeps the rows every step reads dense in memory whatever
 * the cache's capacity (fewer pages touched).  `cap` = total positions (prefix + the stream cache's rows); the
 * new token is written at stream index L0 - T0.  L0 comes from *d_L0 when d_L0 is not NULL (graph replays),
 * else from the argument.  T0 = 0 is ns_decode_attention(_dev).  The output bits do not depend on where a
 * row is stored (same values, same order).  window > 0 (opt-in; 0 = the reference's unbounded attention) attends
 * to the last `window` positions only, [max(0, L0 + 1 - window), L0]: a sliding-window approximation that bounds
 * the per-step KV traffic (NOT the reference's max_context, which re-runs a trimmed context). */
int ns_decode_attention_prefix(const void* d_qkv, int64_t qkv_stride, void* d_k_cache, void* d_v_cache,
                               int64_t cache_b_stride, int64_t cache_h_stride, int64_t cache_chunk_stride,
                               const void* d_k_prefix, const void* d_v_prefix, int64_t prefix_h_stride, int T0, int B,
                               int H, int D, int L0, const int32_t* d_L0, int cap, int window, void* d_out,
                               int64_t out_stride, float scale, void* hip_stream);

/* ns_decode_attention_prefix over an fp8 KV cache (OCP e4m3fn bytes, element layout as above with 1-byte
 * elements): half the HBM bytes of the fp16 cache.  The new token's k/v are quantised (saturated to +-448,
 * round to nearest even) before they are stored and used.  q, scores and the softmax stay fp16/fp32; rows
 * are split by key count only (64-row chunks), so the output is batch-invariant too.  An opt-in numerics
 * mode: logits differ from the fp16 cache's at the fp8 quantisation level.
 * Non-finite k/v (every entry point that converts: this one, ns_decode_attention_ex / _paged / _paged_chunk with
 * NS_KV_FP8, the page store of ns_seq_attention_ragged, ns_quantize_fp8): +-inf saturate to +-448, -0 keeps its sign,
 * and a NaN is stored as an e4m3 NaN byte (0x7F or 0xFF, both NaN to every reader) -- a poisoned row (the NaN rows
 * below, NaN hidden rows of an out-of-range token id) stays NaN in the cache, so every later step of that stream
 * gives NaN output rows, as with the fp16 cache, and no other stream is affected. */
int ns_decode_attention_fp8(const void* d_qkv, int64_t qkv_stride, void* d_k_cache, void* d_v_cache,
                            int64_t cache_b_stride, int64_t cache_h_stride, int64_t cache_chunk_stride,
                            const void* d_k_prefix, const void* d_v_prefix, int64_t prefix_h_stride, int T0, int B,
                            int H, int D, int L0, const int32_t* d_L0, int cap, int window, void* d_out,
                            int64_t out_stride, float scale, void* hip_stream);

/* KV element formats of ns_decode_attention_ex */
#define NS_KV_FP16 0
#define NS_KV_FP8 1

/* ns_decode_attention_prefix (kv_format NS_KV_FP16) / ns_decode_attention_fp8 (NS_KV_FP8) with an optional
 * per-stream end: stream b is skipped if d_done is not NULL and bit 0 of d_done[b * done_stride] is set (uint32
 * words; e.g. the flags word of the coder state, NS_ST_DONE -- encode), or if d_stop is not NULL and the cache
 * length L0 >= d_stop[b] (int32; the position after which a decode needs no more logits): no KV append, no cache
 * read, its output row left as it was.  Both are read when the kernel runs (L0 from d_L0 on graph replays), so one
 * captured hipGraph serves every step while streams finish.  The other streams' outputs are the same bits with or without the flags (a stream's row split depends
 * on its key count only): a lockstep batch whose covers differ in length (peaked, trained-LM rows) stops paying
 * the finished streams' cache reads. */
int ns_decode_attention_ex(const void* d_qkv, int64_t qkv_stride, void* d_k_cache, void* d_v_cache,
                           int64_t cache_b_stride, int64_t cache_h_stride, int64_t cache_chunk_stride,
                           const void* d_k_prefix, const void* d_v_prefix, int64_t prefix_h_stride, int T0, int B,
                           int H, int D, int L0, const int32_t* d_L0, int cap, int window, int kv_format,
                           const uint32_t* d_done, int64_t done_stride, const int32_t* d_stop, void* d_out,
                           int64_t out_stride, float scale, void* hip_stream);

/* ns_decode_attention_ex over a PAGED cache with a cache length PER STREAM (round 6: slot refill and growth
 * without a copy).  Stream b's rows live in 32-position pages: d_page_table[b * table_stride + c] (uint64; the table
 * 8-byte aligned, so a row range of a larger table is a table too) is the
 * device address (16-byte aligned; 0 = none) of the page holding its stream rows 32c .. 32c + 31, i.e. positions
 * T0 + 32c ...; this layer's block of the page starts `layer_offset` elements after that address and holds
 * [K|V][H][32][D] in the kv_format's element type (K at +0, V at +H*32*D; the pool decides where the layers of a page
 * live: layer * 2*H*32*D for pages holding every layer back to back, layer * SEG * 2*H*32*D for segments of SEG pages
 * stored layer-major).  d_lens[b] (int32) = positions already cached for stream b
 * (the new token is written at position d_lens[b] and attended with positions 0 .. d_lens[b]); positions < T0 come
 * from the shared prefix as in ns_decode_attention_prefix.  Only table entries 0 .. max_chunks-1 are read; a stream
 * whose new-token page is missing gets NaN output rows (the coder rejects them) and writes nothing.  d_done / d_stop
 * skip finished streams as in ns_decode_attention_ex (the stop test compares d_lens[b]).  A pair's rows are split
 * by its own key count and merged in the same order as the lockstep kernels: for the same cache contents the output
 * bits equal ns_decode_attention_ex's, whatever the batch, the other streams' lengths or where the pages live.
 * Replaces the reference's per-message cache of code_base/arithmetic.py:96-122 (each message its own loop). */
int ns_decode_attention_paged(const void* d_qkv, int64_t qkv_stride, const uint64_t* d_page_table,
                              int64_t table_stride, int max_chunks, int64_t layer_offset, const void* d_k_prefix,
                              const void* d_v_prefix, int64_t prefix_h_stride, int T0, int B, int H, int D,
                              const int32_t* d_lens, int window, int kv_format, const uint32_t* d_done,
                              int64_t done_stride, const int32_t* d_stop, void* d_out, int64_t out_stride, float scale,
                              void* hip_stream);

/* ns_decode_attention_paged for the next C tokens of every stream in ONE launch (1 <= C <= 16): the decoder of a
 * cover knows every token before its first step, so a stream's K/V pages are read once per C tokens instead of once
 * per token.  d_qkv fp16 [B*C, qkv_stride] and d_out fp16 [B*C, out_stride]: stream b's query i is row b*C + i.
 * d_count (int32 [B], device) = the new rows n_b of stream b, clamped to C; n_b <= 0 leaves the stream untouched.
 * With L = d_lens[b], the call stores the k/v of rows i < n_b at positions L + i of b's pages (the one-token append's
 * values: fp16 bit copies, fp8 the same conversion) and writes, for each i < n_b, the output row of query i over
 * positions 0 .. L + i.  Output rows i >= n_b are never written; d_lens is not advanced (the caller adds d_count).
 * Output row (b, i) and every stored page byte equal, bit for bit, what ns_decode_attention_paged produces when
 * called i + 1 times in a row on the successive qkv rows with d_lens[b] = L, L + 1, ...: every query keeps the row
 * split of its own key count (it may change inside a chunk), the chunk order, the per-row-group online softmax and
 * the merge order of the one-token kernel.  There is no d_done / d_stop: d_count says who runs.
 * Only table entries 0 .. max_chunks-1 are read.  A stream one of whose pages for rows L .. L + n_b - 1 is zero,
 * misaligned or at a chunk >= max_chunks gets NaN in its n_b output rows and writes no page byte; a zero or
 * misaligned entry of an already cached row is not read either and gives NaN rows.
 * Returns NS_ERR_CONFIG for C outside [1, 16] or D != 64, NS_ERR_UNSUPPORTED for window > 0. */
int ns_decode_attention_paged_chunk(const void* d_qkv, int64_t qkv_stride, const uint64_t* d_page_table,
                                    int64_t table_stride, int max_chunks, int64_t layer_offset, const void* d_k_prefix,
                                    const void* d_v_prefix, int64_t prefix_h_stride, int T0, int B, int H, int D,
                                    const int32_t* d_lens, int window, int kv_format, int C, const int32_t* d_count,
                                    void* d_out, int64_t out_stride, float scale, void* hip_stream);

/* Causal attention over B whole sequences of T tokens (positions 0..T-1, no cache): the prefill of the shared
 * context (code_base/arithmetic.py:115-122, the first call), the guard's scoring forward
 * (src/neuralstego/metrics/lm_scorer.py:121-131) and the src provider's max_context window forward
 * (src/neuralstego/lm/arithmetic.py:45-74).  d_qkv fp16 [B*T, qkv_stride] (row b*T + t; q, k, v column blocks as in
 * ns_decode_attention), d_out fp16 [B*T, out_stride].  Flash attention on the 16x16x32 f16 MFMA with an fp32
 * online softmax and P rounded to fp16 for the PV product; each output row depends on its own sequence only
 * (batch-invariant).  D must be 64. */
int ns_seq_attention(const void* d_qkv, int64_t qkv_stride, void* d_out, int64_t out_stride, int B, int T, int H,
                     int D, float scale, void* hip_stream);

/* ns_seq_attention over n_seq sequences of DIFFERENT lengths packed back to back, with the K/V of every sequence
 * optionally written into that stream's KV pages: the prefill of one context PER message
 * (src/neuralstego/api.py:707-747, a seed text per stego_encode call).
 *   d_qkv       fp16 [R, qkv_stride], d_out fp16 [R, out_stride]; sequence s is rows d_seq_start[s] ..
 *               d_seq_start[s + 1] - 1 (d_seq_start: int32 [n_seq + 1], device, ascending, last = R).
 *   d_blocks    int32 [nblk][2], device: (sequence, 64-query block) for every block of every sequence, each once,
 *               longest (highest block index) first; the grid is nblk x H.  The host knows every length and builds
 *               the list.  An entry that names no block inside the R rows is skipped.
 * Same arithmetic, block order and MFMA chains as ns_seq_attention: a sequence's output rows are the bits of
 * ns_seq_attention(B = 1, T = its length) on its own rows, whatever else is packed around it; a workgroup reads
 * rows of its own sequence only (row clamps stay inside it).
 * d_page_table != NULL: sequence s's row r (r < its length) is also stored at page
 * d_page_table[d_seq_slot[s] * table_stride + r / 32] (entries 0 .. max_chunks-1; d_seq_slot int32 [n_seq], values in
 * [0, n_slots)), at layer_offset + [K|V][H][32][D] as ns_decode_attention_paged reads it: NS_KV_FP16 copies the qkv
 * values, NS_KV_FP8 converts them as the decode step's append does, so a prefilled row equals an appended one.
 * Every (sequence, head, row) is written exactly once, by the workgroup of the row's own block; rows of a zero (or
 * misaligned) table entry, of a chunk >= max_chunks or of a slot outside [0, n_slots) are not stored.  d_page_table
 * NULL: attention only (the remaining arguments are ignored).  D must be 64. */
int ns_seq_attention_ragged(const void* d_qkv, int64_t qkv_stride, void* d_out, int64_t out_stride,
                            const int32_t* d_seq_start, int n_seq, int R, const int32_t* d_blocks, int nblk, int H,
                            int D, float scale, const uint64_t* d_page_table, int64_t table_stride, int max_chunks,
                            const int32_t* d_seq_slot, int n_slots, int64_t layer_offset, int kv_format,
                            void* hip_stream);

/* ns_seq_attention_ragged CONTINUED from KV pages: a context whose first rows another prefill already
 * stored (a common prefix of different contexts, lm/kvpages.py) is run from its first new row on.
 *   d_seq_past  int32 [n_seq], device: sequence s has d_seq_past[s] rows -- >= 0 and a multiple of 64 -- in the first
 *               d_seq_past[s] / 32 pages of its table row; its d_seq_start[s + 1] - d_seq_start[s] packed rows are
 *               its ABSOLUTE rows d_seq_past[s] .., and a d_blocks entry (s, j) names the 64 new queries from absolute
 *               row d_seq_past[s] + 64 j.
 * Key blocks below d_seq_past[s] / 64 are staged from the pages (16-byte loads of the bytes an earlier launch stored),
 * the others from the packed rows; masks are absolute and the block order, the online softmax and the MFMA chains
 * are those of ns_seq_attention_ragged (one body).  fp16 pages hold bit copies of the qkv values, so the output rows
 * and the stored rows equal, bit for bit, those of the whole sequence run at once, and d_seq_past all zero gives
 * ns_seq_attention_ragged's result.  New rows are stored at their absolute row (each (sequence, head, row) exactly
 * once); pages below d_seq_past[s] / 32 are never written.
 * Returns NS_ERR_UNSUPPORTED for NS_KV_FP8 (fp8 pages are converted values: no exact continuation exists) and
 * NS_ERR_CONFIG for D != 64, a NULL d_page_table or a NULL d_seq_past.  A sequence whose d_seq_past is negative or no
 * multiple of 64, whose past pages reach beyond max_chunks (or whose slot lies outside [0, n_slots)), or one of whose
 * past table entries is zero or misaligned is skipped whole: no row or page of it is read, no output row and no page
 * written. */
int ns_seq_attention_ragged_past(const void* d_qkv, int64_t qkv_stride, void* d_out, int64_t out_stride,
                                 const int32_t* d_seq_start, const int32_t* d_seq_past, int n_seq, int R,
                                 const int32_t* d_blocks, int nblk, int H, int D, float scale,
                                 const uint64_t* d_page_table, int64_t table_stride, int max_chunks,
                                 const int32_t* d_seq_slot, int n_slots, int64_t layer_offset, int kv_format,
                                 void* hip_stream);

/* The head rows of one KV page into another, for many (source, destination) pairs in one launch: a context's KV
 * pages shared among the messages that carry it -- the context's last, partly filled page is copied into the first
 * own page of every holder, which that holder then appends into (a shared page is never an append target).
 * For i < n and every layer l < n_layer: copy rows 0 .. d_rows[i]-1 of K and of V, every head, from the page at
 * d_src[i] to the page at d_dst[i]  (page = address of its layer-0 block; a layer's block is [K|V][H][32][D] in
 * the kv_format's element type, layer l at + l*layer_stride elements, as ns_decode_attention_paged reads it).
 * Bytes are copied as they are (fp16 or fp8).  Rows >= d_rows[i] of the destination, and every other byte, are
 * not written.  An entry with a zero or misaligned address, d_rows[i] outside [0, 32], or src == dst is skipped.
 * The caller keeps destinations distinct.  n == 0 returns NS_OK without a launch.  D must be 64. */
int ns_kv_copy_rows(const uint64_t* d_src, const uint64_t* d_dst, const int32_t* d_rows, int n, int n_layer,
                    int64_t layer_stride, int H, int D, int kv_format, void* hip_stream);

/* fp16 [n] -> fp8 e4m3fn [n] with the attention's conversion (n % 4 == 0, 8-byte aligned). */
int ns_quantize_fp8(const void* d_src, void* d_dst, int64_t n, void* hip_stream);

#ifdef __cplusplus
}
#endif

#endif /* NSG_ATTN_H */
