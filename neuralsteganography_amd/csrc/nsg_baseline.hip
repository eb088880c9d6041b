// nsg_baseline.hip -- the fixed-block baseline coders (include/nsg_baseline.h): the Huffman coder of
// code_base/huffman_baseline.py + huffman.py and the bins coder of code_base/block_baseline.py, one step for B
// streams.  One workgroup of one wave per stream: the row is streamed once with 16-byte loads into an LDS
// candidate buffer (Huffman: the K = 2^block leaders by threshold filtering and bitonic compaction; bins: one
// 64-bit maximum per bin), the canonical row sum is taken over the row again (exact_row_sum, nsg_common.h), and
// lane 0 replays heapq's own sift sequence on LDS arrays.  Canonical arithmetic must stay bit-identical to
// tests/baseline_cases.py (which calls the oracle's or_exp_canon / or_row_sum).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "nsg_host.h"
#include "../../include/nsg_baseline.h"

#pragma clang fp contract(off)

namespace nsg {

constexpr int BL_CAP = 1024;  // candidate keys per stream (8 B each): 8 KiB of LDS per workgroup
constexpr int BL_MAXK = 256;  // 2^8 leaders / bins at most
enum { BL_HUFFMAN = 0, BL_BINS = 1 };

struct BaselineArgs {
    int block;                // bits per block
    int K;                    // 2^block
    const uint8_t* word2bin;  // bins: [V]
    const uint8_t* sent_end;  // NS_STEP_FINISH_SENT: [V]
};

// Byte offsets of the Huffman arrays inside the candidate buffer, after the K <= 256 ranked keys (2 KiB).
constexpr int HF_BASE = BL_MAXK * 8;
constexpr int HF_W = HF_BASE;               // float  w[511]: node weights (leaves 0..K-1, merged K..2K-2)
constexpr int HF_HEAP = HF_W + 2048;        // uint16 heap[256]: heapq's list, as node indices
constexpr int HF_LEFT = HF_HEAP + 512;      // uint16 left[255]: of node K + i
constexpr int HF_RIGHT = HF_LEFT + 512;     // uint16 right[255]
constexpr int HF_PARENT = HF_RIGHT + 512;   // uint16 parent[511]: parent | 0x8000 when the node is a right child
constexpr int HF_DEPTH = HF_PARENT + 1024;  // uint8  depth[511]: code lengths (statistics)
constexpr int HF_BITS = HF_DEPTH + 512;     // uint8  bits[256]: the code being emitted (decode)
constexpr int HF_SEL = HF_BITS + 256;       // int32  sel, int32 nbits_used
static_assert(HF_SEL + 8 <= BL_CAP * 8, "Huffman arrays must fit the candidate buffer");

// Descending bitonic sort of keys[0, n), n a power of two >= 64, by one wave (the workgroup).
__device__ __forceinline__ void bitonic_desc(uint64_t* keys, int n, int lane) {
    for (int k = 2; k <= n; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = lane; t < (n >> 1); t += WAVE) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
                const int l = i | j;
                const uint64_t a = keys[i], c = keys[l];
                const bool desc = (i & k) == 0;
                if ((a < c) == desc) {
                    keys[i] = c;
                    keys[l] = a;
                }
            }
            __syncthreads();
        }
    }
}

// keys[0, count) -> the min(count, K) largest, sorted descending; returns the new count.  Key 0 (no id has it) pads.
__device__ __forceinline__ int compact_top(uint64_t* keys, int count, int K, int lane) {
    int n = WAVE;
    while (n < count) n <<= 1;
    for (int t = count + lane; t < n; t += WAVE) keys[t] = 0;
    __syncthreads();
    bitonic_desc(keys, n, lane);
    return min(count, K);
}

// One pass over the row: the K largest (value desc, id asc) keys of the ids that are not banned, sorted, into
// keys[0, K).  `bad` is set in lanes that saw a NaN or +inf.  K <= 256 <= valid ids.
template <typename T>
__device__ __forceinline__ void select_top(const StepParams& p, const RowReader& rd, int K, uint64_t* keys, int lane,
                                           bool& bad) {
    constexpr int W = Elem<T>::W;
    const int nvec = (p.V + W - 1) / W;
    int count = 0;
    uint64_t thr = 0;  // K-th largest key so far (0: fewer than K seen)
    for (int base = 0; base < nvec; base += WAVE) {
        if (count + WAVE * W > BL_CAP) {
            count = compact_top(keys, count, K, lane);
            if (count == K) thr = keys[K - 1];
        }
        const int v = base + lane;
        float x[W];
        if (v < nvec) {
            Elem<T>::unpack(rd.vec(v), x);
        } else {
#pragma unroll
            for (int q = 0; q < W; ++q) x[q] = 0.0f;
        }
#pragma unroll
        for (int q = 0; q < W; ++q) {
            const int j = v * W + q;
            const bool valid = v < nvec && j < p.V && !is_banned(p, j);
            bad |= valid && !(x[q] < __builtin_inff());
            const uint64_t key = make_key(x[q], (uint32_t)j);
            const bool pass = valid && key > thr;
            const uint64_t m = ballot(pass);
            if (pass) keys[count + lanes_below(m)] = key;
            count += popc64(m);
        }
    }
    (void)compact_top(keys, count, K, lane);
}

// heapq._siftdown(heap, 0, pos) on node indices ordered by `<` of their fp32 weights
__device__ __forceinline__ void hq_siftdown(uint16_t* heap, const float* w, int pos) {
    const uint16_t item = heap[pos];
    const float wi = w[item];
    while (pos > 0) {
        const int pp = (pos - 1) >> 1;
        const uint16_t par = heap[pp];
        if (wi < w[par]) {
            heap[pos] = par;
            pos = pp;
            continue;
        }
        break;
    }
    heap[pos] = item;
}
// heapq.heappop: the last element replaces the root and sinks to a leaf along the smaller child (the right one
// unless left < right), then sifts down from there -- heapq._siftup
__device__ __forceinline__ int hq_pop(uint16_t* heap, const float* w, int& n) {
    const uint16_t last = heap[--n];
    if (n == 0) return last;
    const uint16_t ret = heap[0];
    int pos = 0, child = 1;
    while (child < n) {
        const int r = child + 1;
        if (r < n && !(w[heap[child]] < w[heap[r]])) child = r;
        heap[pos] = heap[child];
        pos = child;
        child = 2 * pos + 1;
    }
    heap[pos] = last;
    hq_siftdown(heap, w, pos);
    return ret;
}

template <typename T, int MODE, bool DECODE>
__global__ __launch_bounds__(WAVE) void baseline_kernel(StepParams p, BaselineArgs a) {
    __shared__ uint64_t s_keys[BL_CAP];
    char* const lds = (char*)s_keys;
    const int lane = threadIdx.x;
    const int b = __builtin_amdgcn_readfirstlane((int)blockIdx.x);
    if (b >= p.B) return;
    const ns_stream_state st = p.state[b];
    if (st.flags & NS_ST_DONE) return;
    int64_t nbits = 0;
    bool finishing = false;
    if (!DECODE) {
        nbits = p.nbits[b];
        if (st.bit_pos >= nbits) {
            if (!(p.flags & NS_STEP_FINISH_SENT)) {
                if (lane == 0) p.state[b].flags = st.flags | NS_ST_DONE;
                return;
            }
            finishing = true;  // huffman_baseline.py:36-38, block_baseline.py:54-56: top-1 until a sentence end
        }
    } else if (decode_skipped(p, b, st.ntokens)) {
        return;
    }
    const char* rowc = (const char*)p.logits + (int64_t)b * p.ld * (int64_t)sizeof(T);
    const RowReader rd(rowc, (uint32_t)(p.ld * (int64_t)sizeof(T)));
    const int K = a.K;
    bool bad = false;

    if (MODE == BL_BINS && !finishing) {
        constexpr int W = Elem<T>::W;
        const int nvec = (p.V + W - 1) / W;
        for (int t = lane; t < K; t += WAVE) s_keys[t] = 0;
        __syncthreads();
        for (int v = lane; v < nvec; v += WAVE) {
            float x[W];
            Elem<T>::unpack(rd.vec(v), x);
#pragma unroll
            for (int q = 0; q < W; ++q) {
                const int j = v * W + q;
                if (j < p.V) {
                    const bool ban = is_banned(p, j);
                    bad |= !ban && !(x[q] < __builtin_inff());
                    // a banned id ranks after every other id: high word 0, below the key of any value
                    const uint64_t key = ban ? (uint64_t)(0xFFFFFFFFu - (uint32_t)j) : make_key(x[q], (uint32_t)j);
                    const int bin = a.word2bin[j] & (K - 1);
                    if (key > s_keys[bin]) atomicMax((unsigned long long*)&s_keys[bin], (unsigned long long)key);
                }
            }
        }
        __syncthreads();
        // a bin that is empty, all banned or led by -inf cannot carry a block
        for (int t = lane; t < K; t += WAVE) {
            const uint64_t k = s_keys[t];
            bad |= (uint32_t)(k >> 32) == 0u || key_val(k) == -__builtin_inff();
        }
    } else {
        select_top<T>(p, rd, finishing ? 1 : K, s_keys, lane, bad);
        const int kk = finishing ? 1 : K;
        for (int t = lane; t < kk; t += WAVE) bad |= key_val(s_keys[t]) == -__builtin_inff();
    }

    if (ballot(bad) != 0ull) {
        if (lane == 0) {
            p.state[b].flags = st.flags | NS_ST_ERR_RANGE | NS_ST_DONE;
            if (p.trace) {
                ns_step_trace tr = {K, K, -1, -1, -1, 0, 0.0};
                p.trace[b] = tr;
            }
        }
        return;
    }

    if (finishing) {
        if (lane == 0) {
            const int32_t token = (int32_t)key_id(s_keys[0]);
            ns_stream_state ns = st;
            ns.ntokens = st.ntokens + 1;
            if (a.sent_end[token]) ns.flags |= NS_ST_DONE;
            p.state[b] = ns;
            p.out_token[b] = token;
            if (p.hist && st.ntokens < p.hist_stride) p.hist[(int64_t)b * p.hist_stride + st.ntokens] = token;
            if (p.trace) {
                ns_step_trace tr = {0, 0, 0, 0, token, 0, 0.0};
                p.trace[b] = tr;
            }
        }
        return;
    }

    // ---- decode: the received token's rank / bin, or a divergence (before any further row work)
    int32_t token = -1;
    int sel = -1;
    if (DECODE) {
        token = decode_token(p, b, st.ntokens);
        if (MODE == BL_HUFFMAN) {
            for (int base = 0; base < K; base += WAVE) {
                const int i = base + lane;
                const uint64_t m = ballot(i < K && key_id(s_keys[i]) == (uint32_t)token);
                if (m != 0ull) sel = base + __builtin_ctzll(m);
            }
        } else if (token >= 0 && token < p.V) {
            const int bin = a.word2bin[token] & (K - 1);
            if (key_id(s_keys[bin]) == (uint32_t)token) sel = bin;
        }
        sel = __builtin_amdgcn_readfirstlane(sel);
        if (sel < 0) {
            if (p.ranked) {
                int32_t* out = p.ranked + (int64_t)b * p.ranked_stride;
                for (int i = lane; i < K && i < p.ranked_stride; i += WAVE) out[i] = (int32_t)key_id(s_keys[i]);
                if (lane == 0 && K < p.ranked_stride) out[K] = -1;
            }
            if (lane == 0) {
                p.state[b].flags = st.flags | NS_ST_ERR_DIVERGE | NS_ST_DONE;
                if (p.trace) {
                    ns_step_trace tr = {K, K, -1, -1, -1, 0, 0.0};
                    p.trace[b] = tr;
                }
            }
            return;
        }
    }

    // ---- the row maximum and the canonical row sum
    const bool want_stats = !DECODE && p.stats != nullptr;
    double m = 0.0, S = 0.0;
    if (MODE == BL_HUFFMAN) {
        m = (double)key_val(s_keys[0]);
    } else if (want_stats) {
        float mx = -__builtin_inff();
        for (int t = lane; t < K; t += WAVE) mx = fmaxf(mx, key_val(s_keys[t]));
        m = (double)wave_max(mx);
    }
    if (MODE == BL_HUFFMAN || want_stats) S = exact_row_sum<T>(p, rowc, m, lane, 1.0);

    int used = 0;  // payload bits consumed / code bits emitted
    double logp_sel = 0.0, kl = 0.0;
    if (MODE == BL_HUFFMAN) {
        float* const w = (float*)(lds + HF_W);
        uint16_t* const heap = (uint16_t*)(lds + HF_HEAP);
        uint16_t* const left = (uint16_t*)(lds + HF_LEFT);
        uint16_t* const right = (uint16_t*)(lds + HF_RIGHT);
        uint16_t* const parent = (uint16_t*)(lds + HF_PARENT);
        uint8_t* const depth = (uint8_t*)(lds + HF_DEPTH);
        uint8_t* const cbits = (uint8_t*)(lds + HF_BITS);
        int32_t* const selw = (int32_t*)(lds + HF_SEL);
        for (int i = lane; i < K; i += WAVE)
            w[i] = (float)(exp_canon(((double)key_val(s_keys[i]) - m) * 1.0) / S);
        __syncthreads();
        if (lane == 0) {
            const int root = 2 * K - 2;
            int n = 0;
            for (int i = 0; i < K; ++i) {  // make_heap_from_array: heappush in index order
                heap[n] = (uint16_t)i;
                hq_siftdown(heap, w, n);
                ++n;
            }
            int next = K;
            while (n > 1) {  // merge_nodes
                const int n1 = hq_pop(heap, w, n);
                const int n2 = hq_pop(heap, w, n);
                w[next] = w[n1] + w[n2];
                left[next - K] = (uint16_t)n1;
                right[next - K] = (uint16_t)n2;
                parent[n1] = (uint16_t)next;
                parent[n2] = (uint16_t)(next | 0x8000);
                heap[n] = (uint16_t)next;
                hq_siftdown(heap, w, n);
                ++n;
                ++next;
            }
            if (!DECODE) {
                int node = root;
                int64_t pos = st.bit_pos;
                const uint8_t* pl = p.payload + (int64_t)b * p.payload_stride;
                while (node >= K) {  // huffman_baseline.py:47-52: a bit past the end reads as 0
                    const int bit = pos < nbits ? (pl[pos >> 3] >> (pos & 7)) & 1 : 0;
                    node = bit ? right[node - K] : left[node - K];
                    ++pos;
                }
                selw[0] = node;
                selw[1] = (int)(pos - st.bit_pos);
                if (want_stats) {
                    depth[root] = 0;
                    for (int node2 = root; node2 >= K; --node2) {
                        const uint8_t d = (uint8_t)(depth[node2] + 1);
                        depth[left[node2 - K]] = d;
                        depth[right[node2 - K]] = d;
                    }
                }
            } else {
                int d = 0;
                for (int node = sel; node != root; node = parent[node] & 0x7FFF) ++d;
                int i = d;
                for (int node = sel; node != root; node = parent[node] & 0x7FFF) cbits[--i] = (uint8_t)(parent[node] >> 15);
                selw[0] = sel;
                selw[1] = d;
            }
        }
        __syncthreads();
        sel = selw[0];
        used = selw[1];
        if (want_stats) {
            const double logS = log(S);
            double acc = 0.0;
            for (int i = lane; i < K; i += WAVE) {
                const double logq = -(double)depth[i] * 0.69315;  // huffman_baseline.py:55-56
                const double logp = ((double)key_val(s_keys[i]) - m) - logS;
                acc += exp(logq) * (logq - logp) / 0.69315;
            }
            kl = wave_sum_butterfly(acc);
            logp_sel = ((double)key_val(s_keys[sel]) - m) - logS;
        }
        if (!DECODE) token = (int32_t)key_id(s_keys[sel]);
    } else {
        used = a.block;
        if (!DECODE) {
            const uint8_t* pl = p.payload + (int64_t)b * p.payload_stride;
            int v = 0;
            for (int i = 0; i < a.block; ++i) {  // bits2int of message[i:i+block_size], a short tail zero-padded
                const int64_t pos = st.bit_pos + i;
                if (pos < nbits) v |= ((pl[pos >> 3] >> (pos & 7)) & 1) << i;
            }
            sel = v;
            token = (int32_t)key_id(s_keys[sel]);
            if (want_stats) {
                const double logS = log(S);
                const double logq = -(double)a.block * 0.69315;  // block_baseline.py:69-72
                const double q = exp(logq);
                double acc = 0.0;
                for (int t = lane; t < K; t += WAVE) acc += q * (logq - (((double)key_val(s_keys[t]) - m) - logS)) / 0.69315;
                kl = wave_sum_butterfly(acc);
                logp_sel = ((double)key_val(s_keys[sel]) - m) - logS;
            }
        }
    }

    if (DECODE) {
        // append `used` bits LSB-first at bit_pos: whole bytes are assembled by one lane each
        const int64_t first = st.bit_pos, end = st.bit_pos + used;
        if (end > p.out_stride * 8) {
            if (lane == 0) p.state[b].flags = st.flags | NS_ST_ERR_RANGE | NS_ST_DONE;
            return;
        }
        uint8_t* out = p.out_bits + (int64_t)b * p.out_stride;
        const int64_t byte0 = first >> 3;
        const int64_t nbytes = used > 0 ? ((end - 1) >> 3) - byte0 + 1 : 0;  // <= 33
        if (lane < nbytes) {
            const int64_t by = byte0 + lane;
            uint32_t mask = 0, val = 0;
            for (int q = 0; q < 8; ++q) {
                const int64_t pos = by * 8 + q;
                if (pos >= first && pos < end) {
                    const int i = (int)(pos - first);
                    const uint32_t bit = MODE == BL_HUFFMAN ? ((const uint8_t*)(lds + HF_BITS))[i] : ((uint32_t)sel >> i) & 1u;
                    mask |= 1u << q;
                    val |= bit << q;
                }
            }
            out[by] = (uint8_t)((out[by] & ~mask) | val);
        }
    }

    if (lane == 0) {
        ns_stream_state ns = st;
        ns.bit_pos = st.bit_pos + used;
        ns.ntokens = st.ntokens + 1;
        if (!DECODE) {
            if (ns.bit_pos >= nbits && !(p.flags & NS_STEP_FINISH_SENT)) ns.flags |= NS_ST_DONE;
            p.out_token[b] = token;
            if (p.hist && st.ntokens < p.hist_stride) p.hist[(int64_t)b * p.hist_stride + st.ntokens] = token;
            if (want_stats) {
                double* sa = p.stats + (int64_t)b * 4;
                sa[0] += logp_sel;
                sa[1] += kl;
                sa[3] += 1.0;
            }
        }
        p.state[b] = ns;
        if (DECODE) decode_record(p, b, st.ntokens, ns.bit_pos, token);
        if (p.trace) {
            ns_step_trace tr = {K, K, sel, used, token, 1, S};
            p.trace[b] = tr;
        }
    }
}

}  // namespace nsg

namespace {

int bl_fail(ns_ctx* ctx, int code, const char* msg) {
    if (ctx) ctx->err = msg;
    return code;
}

int bl_prepare(ns_ctx* ctx, nsg::StepParams& p, nsg::BaselineArgs& a, const void* d_logits, int64_t ld, int B,
               int block_size, const int32_t* banned, int nbanned, ns_stream_state* d_state, ns_step_trace* d_trace,
               uint32_t flags) {
    if (!ctx) return NS_ERR_CONFIG;
    if (ctx->dtype != NS_DTYPE_F32 && ctx->dtype != NS_DTYPE_F16)
        return bl_fail(ctx, NS_ERR_CONFIG, "baseline coders take fp32 or fp16 logits rows");
    const int W = ctx->dtype == NS_DTYPE_F16 ? 8 : 4;
    if (!d_logits || !d_state || B < 1 || B > ctx->max_batch) return bl_fail(ctx, NS_ERR_CONFIG, "bad batch or pointer");
    if (ld < ctx->vocab || (ld % W) != 0)
        return bl_fail(ctx, NS_ERR_CONFIG, "ld must be >= vocab and a multiple of 16 bytes");
    if (((uintptr_t)d_logits & 15u) != 0u) return bl_fail(ctx, NS_ERR_CONFIG, "logits must be 16-byte aligned");
    if (block_size < 1 || block_size > 8) return bl_fail(ctx, NS_ERR_CONFIG, "block_size must be within [1, 8]");
    if (nbanned < 0 || nbanned > NS_MAX_BANNED || (nbanned > 0 && !banned))
        return bl_fail(ctx, NS_ERR_CONFIG, "too many banned ids");
    int ban[NS_MAX_BANNED];
    int nb = 0;
    for (int i = 0; i < nbanned; ++i)
        if (banned[i] >= 0 && banned[i] < ctx->vocab) ban[nb++] = banned[i];
    std::sort(ban, ban + nb);
    nb = (int)(std::unique(ban, ban + nb) - ban);
    if ((1 << block_size) > ctx->vocab - nb)
        return bl_fail(ctx, NS_ERR_CONFIG, "2^block_size exceeds the ids left after the ban");
    memset(&p, 0, sizeof p);
    p.logits = d_logits;
    p.ld = ld;
    p.B = B;
    p.V = ctx->vocab;
    p.inv_temp = 1.0;
    p.nbanned = nb;
    for (int i = 0; i < nb; ++i) p.banned[i] = ban[i];
    p.flags = flags;
    p.state = d_state;
    p.trace = d_trace;
    p.ranked = ctx->ranked;
    p.ranked_stride = ctx->ranked_stride;
    a.block = block_size;
    a.K = 1 << block_size;
    a.word2bin = nullptr;
    a.sent_end = ctx->sent_end;
    return NS_OK;
}

template <int MODE, bool DECODE>
int bl_launch(ns_ctx* ctx, const nsg::StepParams& p, const nsg::BaselineArgs& a, void* hip_stream) {
    const dim3 g(p.B), blk(nsg::WAVE);
    if (ctx->dtype == NS_DTYPE_F16)
        hipLaunchKernelGGL((nsg::baseline_kernel<_Float16, MODE, DECODE>), g, blk, 0, (hipStream_t)hip_stream, p, a);
    else
        hipLaunchKernelGGL((nsg::baseline_kernel<float, MODE, DECODE>), g, blk, 0, (hipStream_t)hip_stream, p, a);
    if (hipGetLastError() != hipSuccess) return bl_fail(ctx, NS_ERR_HIP, "baseline step: launch failed");
    return NS_OK;
}

template <int MODE>
int bl_encode(ns_ctx* ctx, const void* d_logits, int64_t ld, int B, int block_size, const uint8_t* d_word2bin,
              const uint8_t* d_payload, int64_t payload_stride, const int64_t* d_payload_nbits,
              ns_stream_state* d_state, int32_t* d_out_token, int32_t* d_token_hist, int64_t hist_stride,
              const int32_t* banned, int nbanned, double* d_stats, ns_step_trace* d_trace, uint32_t step_flags,
              void* hip_stream) {
    nsg::StepParams p;
    nsg::BaselineArgs a;
    const int rc = bl_prepare(ctx, p, a, d_logits, ld, B, block_size, banned, nbanned, d_state, d_trace, step_flags);
    if (rc != NS_OK) return rc;
    if (!d_payload || !d_payload_nbits || !d_out_token || payload_stride < 0)
        return bl_fail(ctx, NS_ERR_CONFIG, "baseline encode step: null payload/out pointer");
    if (MODE == nsg::BL_BINS && !d_word2bin) return bl_fail(ctx, NS_ERR_CONFIG, "bins step: null word-to-bin table");
    if ((step_flags & NS_STEP_FINISH_SENT) && !ctx->sent_end)
        return bl_fail(ctx, NS_ERR_CONFIG, "NS_STEP_FINISH_SENT needs ns_set_sentence_end");
    if (d_stats && ((uintptr_t)d_stats & 7u)) return bl_fail(ctx, NS_ERR_CONFIG, "misaligned statistics array");
    a.word2bin = d_word2bin;
    p.payload = d_payload;
    p.payload_stride = payload_stride;
    p.nbits = d_payload_nbits;
    p.out_token = d_out_token;
    p.hist = d_token_hist;
    p.hist_stride = d_token_hist ? hist_stride : 0;
    p.stats = d_stats;
    return bl_launch<MODE, false>(ctx, p, a, hip_stream);
}

template <int MODE>
int bl_decode(ns_ctx* ctx, const void* d_logits, int64_t ld, int B, int block_size, const uint8_t* d_word2bin,
              const int32_t* d_in_token, const uint8_t* d_active, const int32_t* d_tokens, int64_t tok_stride,
              const int32_t* d_length, int64_t* d_counts, int64_t counts_stride, int32_t* d_out_token,
              bool streams, ns_stream_state* d_state, uint8_t* d_out_bits, int64_t out_stride, const int32_t* banned,
              int nbanned, ns_step_trace* d_trace, uint32_t step_flags, void* hip_stream) {
    nsg::StepParams p;
    nsg::BaselineArgs a;
    const int rc = bl_prepare(ctx, p, a, d_logits, ld, B, block_size, banned, nbanned, d_state, d_trace, step_flags);
    if (rc != NS_OK) return rc;
    if (!d_out_bits || out_stride < 1) return bl_fail(ctx, NS_ERR_CONFIG, "baseline decode step: null out pointer");
    if (MODE == nsg::BL_BINS && !d_word2bin) return bl_fail(ctx, NS_ERR_CONFIG, "bins step: null word-to-bin table");
    a.word2bin = d_word2bin;
    if (streams) {
        if (!d_tokens || !d_length || !d_counts || !d_out_token || tok_stride < 1 || counts_stride < 1 ||
            ((uintptr_t)d_tokens & 3u) || ((uintptr_t)d_length & 3u) || ((uintptr_t)d_counts & 7u))
            return bl_fail(ctx, NS_ERR_CONFIG, "baseline decode step: bad token table");
        p.dec_tokens = d_tokens;
        p.dec_tok_stride = tok_stride;
        p.dec_length = d_length;
        p.dec_counts = d_counts;
        p.dec_counts_stride = counts_stride;
        p.out_token = d_out_token;
    } else {
        if (!d_in_token) return bl_fail(ctx, NS_ERR_CONFIG, "baseline decode step: null token pointer");
        p.in_token = d_in_token;
        p.active = d_active;
    }
    p.out_bits = d_out_bits;
    p.out_stride = out_stride;
    return bl_launch<MODE, true>(ctx, p, a, hip_stream);
}

}  // namespace

extern "C" {

int ns_huffman_encode_step(ns_ctx* ctx, const void* d_logits, int64_t ld, int B, int block_size,
                           const uint8_t* d_payload, int64_t payload_stride, const int64_t* d_payload_nbits,
                           ns_stream_state* d_state, int32_t* d_out_token, int32_t* d_token_hist, int64_t hist_stride,
                           const int32_t* banned, int nbanned, double* d_stats, ns_step_trace* d_trace,
                           uint32_t step_flags, void* hip_stream) {
    return bl_encode<nsg::BL_HUFFMAN>(ctx, d_logits, ld, B, block_size, nullptr, d_payload, payload_stride,
                                      d_payload_nbits, d_state, d_out_token, d_token_hist, hist_stride, banned,
                                      nbanned, d_stats, d_trace, step_flags, hip_stream);
}

int ns_huffman_decode_step(ns_ctx* ctx, const void* d_logits, int64_t ld, int B, int block_size,
                           const int32_t* d_in_token, const uint8_t* d_active, ns_stream_state* d_state,
                           uint8_t* d_out_bits, int64_t out_stride, const int32_t* banned, int nbanned,
                           ns_step_trace* d_trace, uint32_t step_flags, void* hip_stream) {
    return bl_decode<nsg::BL_HUFFMAN>(ctx, d_logits, ld, B, block_size, nullptr, d_in_token, d_active, nullptr, 0,
                                      nullptr, nullptr, 0, nullptr, false, d_state, d_out_bits, out_stride, banned,
                                      nbanned, d_trace, step_flags, hip_stream);
}

int ns_huffman_decode_step_streams(ns_ctx* ctx, const void* d_logits, int64_t ld, int B, int block_size,
                                   const int32_t* d_tokens, int64_t tok_stride, const int32_t* d_length,
                                   ns_stream_state* d_state, uint8_t* d_out_bits, int64_t out_stride,
                                   int64_t* d_counts, int64_t counts_stride, int32_t* d_out_token,
                                   const int32_t* banned, int nbanned, ns_step_trace* d_trace, uint32_t step_flags,
                                   void* hip_stream) {
    return bl_decode<nsg::BL_HUFFMAN>(ctx, d_logits, ld, B, block_size, nullptr, nullptr, nullptr, d_tokens,
                                      tok_stride, d_length, d_counts, counts_stride, d_out_token, true, d_state,
                                      d_out_bits, out_stride, banned, nbanned, d_trace, step_flags, hip_stream);
}

int ns_bins_encode_step(ns_ctx* ctx, const void* d_logits, int64_t ld, int B, int block_size,
                        const uint8_t* d_word2bin, const uint8_t* d_payload, int64_t payload_stride,
                        const int64_t* d_payload_nbits, ns_stream_state* d_state, int32_t* d_out_token,
                        int32_t* d_token_hist, int64_t hist_stride, const int32_t* banned, int nbanned,
                        double* d_stats, ns_step_trace* d_trace, uint32_t step_flags, void* hip_stream) {
    return bl_encode<nsg::BL_BINS>(ctx, d_logits, ld, B, block_size, d_word2bin, d_payload, payload_stride,
                                   d_payload_nbits, d_state, d_out_token, d_token_hist, hist_stride, banned, nbanned,
                                   d_stats, d_trace, step_flags, hip_stream);
}

int ns_bins_decode_step(ns_ctx* ctx, const void* d_logits, int64_t ld, int B, int block_size,
                        const uint8_t* d_word2bin, const int32_t* d_in_token, const uint8_t* d_active,
                        ns_stream_state* d_state, uint8_t* d_out_bits, int64_t out_stride, const int32_t* banned,
                        int nbanned, ns_step_trace* d_trace, uint32_t step_flags, void* hip_stream) {
    return bl_decode<nsg::BL_BINS>(ctx, d_logits, ld, B, block_size, d_word2bin, d_in_token, d_active, nullptr, 0,
                                   nullptr, nullptr, 0, nullptr, false, d_state, d_out_bits, out_stride, banned,
                                   nbanned, d_trace, step_flags, hip_stream);
}

int ns_bins_decode_step_streams(ns_ctx* ctx, const void* d_logits, int64_t ld, int B, int block_size,
                                const uint8_t* d_word2bin, const int32_t* d_tokens, int64_t tok_stride,
                                const int32_t* d_length, ns_stream_state* d_state, uint8_t* d_out_bits,
                                int64_t out_stride, int64_t* d_counts, int64_t counts_stride, int32_t* d_out_token,
                                const int32_t* banned, int nbanned, ns_step_trace* d_trace, uint32_t step_flags,
                                void* hip_stream) {
    return bl_decode<nsg::BL_BINS>(ctx, d_logits, ld, B, block_size, d_word2bin, nullptr, nullptr, d_tokens,
                                   tok_stride, d_length, d_counts, counts_stride, d_out_token, true, d_state,
                                   d_out_bits, out_stride, banned, nbanned, d_trace, step_flags, hip_stream);
}

}  // extern "C"
