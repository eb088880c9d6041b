// Decode-step attention of the batched GPT-2 forward with the KV append fused in (include/nsg_attn.h).
//
// Reference semantics: Hugging Face GPT2Attention for one new token per stream over the unbounded cache the
// reference keeps (code_base/arithmetic.py:115-122): softmax(q k^T / sqrt(D)) v over positions 0..L0.
//
// Layout: a pair's rows are split over S = 1, 2, 4 or 8 waves by the KEY COUNT alone (att_split), so the
// summation order -- and every output bit -- is the same whatever the batch size; the S partials are merged in
// wave order through LDS.  Lane l holds dims 8*(l&7)..+7 of key row (l>>3) of an 8-row
// chunk, so an 8-lane group reads one 128-byte K (and V) row and the wave reads 1 KiB of contiguous cache per
// 16-byte load instruction.  Scores are reduced inside the 8-lane group; each group keeps its own online
// softmax (running max, sum, 8 accumulator dims) over the rows it saw, and the 8 groups are merged once at the
// end.  fp16 q.k products with fp32 accumulation (v_dot2_f32_f16), exp2 with log2(e) folded into the scale.
// HBM-bound: 2*(L0+1)*128 bytes per (stream, head) read once, non-temporal (the rows are not reused within
// the step).  The new token's k/v come from the qkv registers and are written to the cache by group 0.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "nsg_attn.h"
#include "nsg_coder.h"

namespace nsg {

#ifndef NSG_ATT_ROWS1
#define NSG_ATT_ROWS1 256  // keys per pair up to which one wave takes the whole pair (then 2, 4, 8 waves)
#endif
#ifndef NSG_ATT_HEAD_MAJOR
#define NSG_ATT_HEAD_MAJOR 1  // large batches: a workgroup's 8 pairs are 8 streams of ONE head (shared context rows
                              // then come from the CU's cache), not 8 consecutive (stream, head) pairs; round 5:
                              // 0.2-1.3 % faster at L = 300-1,000 (profiles/r05/attn_head_major_ab/)
#endif
#ifndef NSG_ATT_SMALL_PAIRS
#define NSG_ATT_SMALL_PAIRS 1024  // up to this many (stream, head) pairs: one pair per workgroup
#endif

constexpr int ATT_D = 64;

#ifndef NSG_ATT_LOAD
#define NSG_ATT_LOAD 0  // K/V row loads: 0 = non-temporal (the rows are not reused within the step), 1 = default policy
#endif

template <class R>
__device__ __forceinline__ R att_load(const R* p) {
#if NSG_ATT_LOAD == 1
    return *p;
#else
    return __builtin_nontemporal_load(p);
#endif
}


typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float dot8(f16x8 a, f16x8 b) {
    float s = 0.0f;
    s = __builtin_amdgcn_fdot2(__builtin_shufflevector(a, a, 0, 1), __builtin_shufflevector(b, b, 0, 1), s, false);
    s = __builtin_amdgcn_fdot2(__builtin_shufflevector(a, a, 2, 3), __builtin_shufflevector(b, b, 2, 3), s, false);
    s = __builtin_amdgcn_fdot2(__builtin_shufflevector(a, a, 4, 5), __builtin_shufflevector(b, b, 4, 5), s, false);
    s = __builtin_amdgcn_fdot2(__builtin_shufflevector(a, a, 6, 7), __builtin_shufflevector(b, b, 6, 7), s, false);
    return s;
}

__device__ __forceinline__ void unpack8(f16x8 v, float* f) {
#pragma unroll
    for (int i = 0; i < 8; ++i) f[i] = (float)v[i];
}

// Split of one (stream, head) pair's rows over waves, a function of the key count ONLY (never of the batch):
// S waves take the 32-row chunks w, w + S, ... and their online-softmax partials are merged in wave order.
// Short caches keep one wave per pair (a short row list split eight ways is mostly idle waves); long caches
// use eight, so a lone stream still spreads its rows over a CU.
__device__ __forceinline__ int att_split(int Lk) {
    return Lk <= NSG_ATT_ROWS1 ? 1 : Lk <= 2 * NSG_ATT_ROWS1 ? 2 : Lk <= 4 * NSG_ATT_ROWS1 ? 4 : 8;
}

// K/V storage formats.  A lane holds DPL consecutive dims of one key row, LPR lanes a row, RPI rows per 16-byte
// wave-load, NI wave-loads per 32-row chunk.  The fp16 format is the reference configuration; the fp8 one
// (OCP e4m3fn, saturated to +-448, round to nearest even, NaN kept as the NaN byte; opt-in) halves the cache bytes the
// HBM-bound decode reads.  q stays fp16 either way; scores and the softmax run in fp32.
struct FmtF16 {
    static constexpr int DPL = 8, LPR = 8, RPI = 8, NI = 4;
    typedef _Float16 Elem;
    typedef f16x8 Raw;
    struct Q {
        f16x8 v;
    };
    static __device__ __forceinline__ Q load_q(const _Float16* p) { return Q{*(const f16x8*)p}; }
    static __device__ __forceinline__ Raw from_qkv(const _Float16* p) { return *(const f16x8*)p; }
    static __device__ __forceinline__ float dot(const Q& q, Raw k) { return dot8(q.v, k); }
    static __device__ __forceinline__ void unpack(Raw v, float* f) { unpack8(v, f); }
};

// Saturation to +-448 that keeps a NaN: ordered comparisons are false for NaN, so it passes through to the
// conversion and becomes the e4m3 NaN byte.  (fminf(fmaxf(x, -448), 448) compiles to one v_med3_f32, which returns
// -448 for a NaN operand: a poisoned k/v row -- NaN hidden rows of a bad token id, include/nsg_attn.h -- was stored
// as finite -448s and the stream went on with finite, wrong logits.  +-inf saturate, -0 keeps its sign.)
__device__ __forceinline__ float sat_fp8(float x) {
    x = x > 448.0f ? 448.0f : x;
    return x < -448.0f ? -448.0f : x;
}

__device__ __forceinline__ uint32_t pack4_fp8(float a, float b, float c, float d) {
    // saturate first: the conversion itself does not clamp, and e4m3fn has no infinity
    a = sat_fp8(a);
    b = sat_fp8(b);
    c = sat_fp8(c);
    d = sat_fp8(d);
    int w = __builtin_amdgcn_cvt_pk_fp8_f32(a, b, 0, false);
    w = __builtin_amdgcn_cvt_pk_fp8_f32(c, d, w, true);
    return (uint32_t)w;
}

#ifndef NSG_ATT_DB8
#define NSG_ATT_DB8 0  // 1: fp8 pages keep the register double buffer in multi-pair workgroups too (A/B)
#endif
#ifndef NSG_ATT_DB8_WPE
#define NSG_ATT_DB8_WPE 3  // ... at this many waves per SIMD
#endif
#ifndef NSG_ATT_F8_NI
#define NSG_ATT_F8_NI 2  // 16-row wave-loads per fp8 chunk
#endif

struct FmtF8 {
    static constexpr int DPL = 16, LPR = 4, RPI = 16, NI = NSG_ATT_F8_NI;
    typedef uint8_t Elem;
    typedef u32x4 Raw;
    struct Q {
        f16x8 a, b;  // the lane's 16 query dims, fp16
    };
    static __device__ __forceinline__ Q load_q(const _Float16* p) {
        return Q{*(const f16x8*)p, *(const f16x8*)(p + 8)};
    }
    static __device__ __forceinline__ Raw from_qkv(const _Float16* p) {  // the new token's k or v, quantised
        const f16x8 a = *(const f16x8*)p, b = *(const f16x8*)(p + 8);
        Raw r;
        r[0] = pack4_fp8((float)a[0], (float)a[1], (float)a[2], (float)a[3]);
        r[1] = pack4_fp8((float)a[4], (float)a[5], (float)a[6], (float)a[7]);
        r[2] = pack4_fp8((float)b[0], (float)b[1], (float)b[2], (float)b[3]);
        r[3] = pack4_fp8((float)b[4], (float)b[5], (float)b[6], (float)b[7]);
        return r;
    }
    // v (fp8, exact in f32) for the PV accumulation: one v_cvt_pk_f32_fp8 per 2 values
    static __device__ __forceinline__ void unpack(Raw v, float* f) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const auto lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)v[i], false);
            const auto hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)v[i], true);
            f[4 * i + 0] = lo[0];
            f[4 * i + 1] = lo[1];
            f[4 * i + 2] = hi[0];
            f[4 * i + 3] = hi[1];
        }
    }
    // q.k: every e4m3 value is exact in fp16, so k goes fp8 -> fp16 pairs (v_cvt_scalef32_pk_f16_fp8, scale 1) and
    // the products run on v_dot2c_f32_f16 like the fp16 cache's, two dims per instruction
    static __device__ __forceinline__ float dot(const Q& q, Raw k) {
        const f16x2 qp[8] = {__builtin_shufflevector(q.a, q.a, 0, 1), __builtin_shufflevector(q.a, q.a, 2, 3),
                             __builtin_shufflevector(q.a, q.a, 4, 5), __builtin_shufflevector(q.a, q.a, 6, 7),
                             __builtin_shufflevector(q.b, q.b, 0, 1), __builtin_shufflevector(q.b, q.b, 2, 3),
                             __builtin_shufflevector(q.b, q.b, 4, 5), __builtin_shufflevector(q.b, q.b, 6, 7)};
        float s = 0.0f;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const f16x2 lo = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8((int)k[i], 1.0f, false);
            const f16x2 hi = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8((int)k[i], 1.0f, true);
            s = __builtin_amdgcn_fdot2(lo, qp[2 * i], s, false);
            s = __builtin_amdgcn_fdot2(hi, qp[2 * i + 1], s, false);
        }
        return s;
    }
};

// Workgroup = 8 waves serving P consecutive pairs (P = 1 for small batches, 8 otherwise; P changes only which
// workgroup computes a pair, not how).  With S = att_split(L0 + 1), the waves form 8/S groups of S; group
// q takes pairs q, q + 8/S, ... of the workgroup, one round per pair, all waves running the same number of
// rounds so the LDS merge's barriers are uniform.
// Positions [0, T0) come from a prefix shared by every stream (kp/vp, head stride ph: the common context,
// stored once), positions [T0, L0] from the stream's own cache at index position - T0.  Same values, same
// order: the output bits do not depend on where a row is stored.
// Which (stream, head) pair slot j of workgroup g serves (-1: none).  Work placement only: the math of a pair does
// not depend on it.
template <int P>
__device__ __forceinline__ int att_pair(int g, int j, int B, int H) {
    if (P > 1 && NSG_ATT_HEAD_MAJOR) {
        const int h = g % H, b = (g / H) * P + j;
        return b < B ? b * H + h : -1;
    }
    const int pair = g * P + j;
    return pair < B * H ? pair : -1;
}

template <class F, int P>
__global__ __launch_bounds__(512) void decode_attn_kernel(const _Float16* __restrict__ qkv, int64_t qkv_stride,
                                                          typename F::Elem* kc, typename F::Elem* vc, int64_t cb,
                                                          int64_t ch, int64_t cz, const typename F::Elem* __restrict__ kp,
                                                          const typename F::Elem* __restrict__ vp, int64_t ph, int T0,
                                                          int B, int H, int L0, const int32_t* __restrict__ L0p,
                                                          int cap, int window,
                                                          const uint32_t* __restrict__ done, int64_t done_stride,
                                                          const int32_t* __restrict__ stop,
                                                          _Float16* __restrict__ out, int64_t out_stride,
                                                          float scale_log2) {
    typedef typename F::Elem E;
    typedef typename F::Raw Raw;
    constexpr int DPL = F::DPL, LPR = F::LPR, RPI = F::RPI, NI = F::NI;
    if (L0p) L0 = __builtin_amdgcn_readfirstlane(*L0p);  // graph replays: the cache length lives on the device
    if (L0 < T0 || L0 >= cap) {  // never write past the cache (the host checks capacity); with a device-side L0
        // the host cannot see an overflow before the launch, so poison this workgroup's output rows: the NaNs
        // reach the logits and the coder rejects them, instead of the next GEMM reusing stale rows
        for (int i = threadIdx.x; i < P * ATT_D; i += blockDim.x) {
            const int pair = att_pair<P>(blockIdx.x, i / ATT_D, B, H);
            if (pair >= 0)
                out[(int64_t)(pair / H) * out_stride + (pair % H) * ATT_D + i % ATT_D] = (_Float16)__builtin_nanf("");
        }
        return;
    }
    __shared__ float s_m[8], s_l[8];
    __shared__ float s_acc[8][ATT_D];
    const int Lk = L0 + 1;
    // attention window (opt-in, 0 = the reference's unbounded cache): keys [s0, L0], s0 = max(0, L0 + 1 - window)
    const int s0 = window > 0 ? max(0, Lk - window) : 0;
    const int S = att_split(Lk - s0);
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int grp = wave / S, wv = wave - grp * S, ngrp = 8 / S;
    const int g = lane / LPR;  // row within an RPI-row slab
    const int c = lane % LPR;  // DPL-dim slice
    const int C = H * ATT_D;
    const int last_cached = L0 > 0 ? L0 - 1 : 0;
    const int rounds = (P + ngrp - 1) / ngrp;
    for (int rd = 0; rd < rounds; ++rd) {
        const int j = grp + rd * ngrp;
        const int pair = j < P ? att_pair<P>(blockIdx.x, j, B, H) : -1;
        // uniform per wave group; a finished stream (done flag bit 0, e.g. the coder state's NS_ST_DONE, or a cache
        // length at its stop position) is skipped: no KV append, no cache read, its output row keeps its old (finite)
        // values, which nothing uses again
        const int sb = pair / H;
        const bool active = pair >= 0 && !(done && (done[(int64_t)sb * done_stride] & 1u)) &&
                            !(stop && L0 >= stop[sb]);
        float m = -1e30f, l = 0.0f;
        float acc[DPL];
#pragma unroll
        for (int d = 0; d < DPL; ++d) acc[d] = 0.0f;
        int b = 0, h = 0;
        if (active) {
            b = pair / H;
            h = pair - b * H;
            const _Float16* qrow = qkv + (int64_t)b * qkv_stride + h * ATT_D + c * DPL;
            const typename F::Q q = F::load_q(qrow);
            const Raw knew = F::from_qkv(qrow + C);
            const Raw vnew = F::from_qkv(qrow + 2 * C);
            // stream rows are addressed by position (index position - T0 folded into the base)
            // stream row j (position T0 + j) at (j / 32) * cz + (j % 32) * D: rows grouped in 32-row chunks, the
            // chunks of all (stream, head) pairs at one position range side by side (cz = chunk plane stride;
            // cz = 32 * D is the plain row-contiguous layout)
            E* kb = kc + (int64_t)b * cb + (int64_t)h * ch + c * DPL;
            E* vb = vc + (int64_t)b * cb + (int64_t)h * ch + c * DPL;
            auto soff = [&](int row) -> int64_t {
                const int jj = row - T0;
                return (int64_t)(jj >> 5) * cz + (int64_t)(jj & 31) * ATT_D;
            };
            const E* kpb = kp + (int64_t)h * ph + c * DPL;
            const E* vpb = vp + (int64_t)h * ph + c * DPL;
            if (g == 0 && wv == 0) {  // KV append of the new token (position L0)
                *(Raw*)(kb + soff(L0)) = knew;
                *(Raw*)(vb + soff(L0)) = vnew;
            }
            // one chunk of RPI*NI rows; GENERAL handles the prefix boundary, the clamp past the cache, rows past
            // Lk and the new token from registers -- an interior chunk (all rows stream rows < L0) skips those
            // selects (same operations on the same values: the bits do not depend on the path).  Small batches
            // (P = 1) issue the next chunk's loads before this chunk's math (register double buffer): a wave's
            // chunks are otherwise one dependent memory round trip each, which is what a lone stream waits on.
            auto load_chunk = [&](int j0, auto general, Raw (&kr)[NI], Raw (&vr)[NI]) {
                constexpr bool GEN = decltype(general)::value;
#pragma unroll
                for (int u = 0; u < NI; ++u) {
                    if constexpr (GEN) {
                        const int row = min(j0 + RPI * u + g, last_cached);
                        const bool pre = row < T0;
                        const E* ka = pre ? kpb + (int64_t)row * ATT_D : kb + soff(row);
                        const E* va = pre ? vpb + (int64_t)row * ATT_D : vb + soff(row);
                        kr[u] = att_load((const Raw*)ka);
                        vr[u] = att_load((const Raw*)va);
                    } else {
                        const int row = j0 + RPI * u + g;
                        const int64_t o = soff(row);
                        kr[u] = att_load((const Raw*)(kb + o));
                        vr[u] = att_load((const Raw*)(vb + o));
                    }
                }
            };
            auto math_chunk = [&](int j0, auto general, Raw (&kr)[NI], Raw (&vr)[NI]) {
                constexpr bool GEN = decltype(general)::value;
                float sc[NI];
                bool valid[NI];
                float mx = m;
#pragma unroll
                for (int u = 0; u < NI; ++u) {
                    const int row = j0 + RPI * u + g;
                    valid[u] = GEN ? row < Lk : true;
                    if (GEN && row == L0) {  // the new token: from registers, not from the cache just written
                        kr[u] = knew;
                        vr[u] = vnew;
                    }
                    float sv = F::dot(q, kr[u]);
#pragma unroll
                    for (int off = 1; off < LPR; off <<= 1) sv += __shfl_xor(sv, off);
                    sc[u] = sv * scale_log2;
                    if (valid[u]) mx = fmaxf(mx, sc[u]);
                }
                const float alpha = exp2f(m - mx);
                l *= alpha;
#pragma unroll
                for (int d = 0; d < DPL; ++d) acc[d] *= alpha;
#pragma unroll
                for (int u = 0; u < NI; ++u) {
                    const float p = valid[u] ? exp2f(sc[u] - mx) : 0.0f;
                    l += p;
                    float v[DPL];
                    F::unpack(vr[u], v);
#pragma unroll
                    for (int d = 0; d < DPL; ++d) acc[d] = fmaf(p, v[d], acc[d]);
                }
                m = mx;
            };
            auto interior = [&](int j0) { return j0 >= T0 && j0 + RPI * NI <= L0; };  // wave-uniform
            const int step = S * RPI * NI;
            Raw kr[NI], vr[NI];
            int j0 = s0 + wv * RPI * NI;
            if constexpr (P > 1) {  // large batches: other waves hide the latency; no second register buffer
                for (; j0 < Lk; j0 += step) {
                    if (interior(j0)) {
                        load_chunk(j0, std::false_type{}, kr, vr);
                        math_chunk(j0, std::false_type{}, kr, vr);
                    } else {
                        load_chunk(j0, std::true_type{}, kr, vr);
                        math_chunk(j0, std::true_type{}, kr, vr);
                    }
                }
            } else {
            Raw kn[NI], vn[NI];
            if (j0 < Lk) {
                if (interior(j0))
                    load_chunk(j0, std::false_type{}, kr, vr);
                else
                    load_chunk(j0, std::true_type{}, kr, vr);
            }
            for (; j0 < Lk; j0 += step) {
                const int j1 = j0 + step;
                if (j1 < Lk) {
                    if (interior(j1))
                        load_chunk(j1, std::false_type{}, kn, vn);
                    else
                        load_chunk(j1, std::true_type{}, kn, vn);
                }
                if (interior(j0))
                    math_chunk(j0, std::false_type{}, kr, vr);
                else
                    math_chunk(j0, std::true_type{}, kr, vr);
#pragma unroll
                for (int u = 0; u < NI; ++u) {
                    kr[u] = kn[u];
                    vr[u] = vn[u];
                }
            }
            }
            // merge the row groups (lanes c, c + LPR, ... hold the same dims)
#pragma unroll
            for (int off = LPR; off < 64; off <<= 1) {
                const float mo = __shfl_xor(m, off);
                const float lo = __shfl_xor(l, off);
                const float mn = fmaxf(m, mo);
                const float fa = exp2f(m - mn), fo = exp2f(mo - mn);
                l = l * fa + lo * fo;
#pragma unroll
                for (int d = 0; d < DPL; ++d) {
                    const float ao = __shfl_xor(acc[d], off);
                    acc[d] = acc[d] * fa + ao * fo;
                }
                m = mn;
            }
        }
        if (S > 1) {  // uniform over the workgroup: hand the S partials of each group to its first wave
            if (active && g == 0) {
#pragma unroll
                for (int d = 0; d < DPL; ++d) s_acc[wave][c * DPL + d] = acc[d];
                if (c == 0) {
                    s_m[wave] = m;
                    s_l[wave] = l;
                }
            }
            __syncthreads();
            if (active && wv == 0) {
                const int w0 = grp * S;
                float mt = s_m[w0];
                for (int w = 1; w < S; ++w) mt = fmaxf(mt, s_m[w0 + w]);
                l = 0.0f;
#pragma unroll
                for (int d = 0; d < DPL; ++d) acc[d] = 0.0f;
                for (int w = 0; w < S; ++w) {
                    const float f = exp2f(s_m[w0 + w] - mt);
                    l += s_l[w0 + w] * f;
#pragma unroll
                    for (int d = 0; d < DPL; ++d) acc[d] += s_acc[w0 + w][c * DPL + d] * f;
                }
            }
            __syncthreads();  // the LDS slots are reused by the next round
        }
        if (active && wv == 0 && g == 0) {
            const float inv = 1.0f / l;
#pragma unroll
            for (int h8 = 0; h8 < DPL / 8; ++h8) {
                f16x8 o;
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    float t = acc[h8 * 8 + i] * inv;
                    asm volatile("" : "+v"(t));  // no fused multiply-convert (one rounding) in some variants only
                    o[i] = (_Float16)t;
                }
                *(f16x8*)(out + (int64_t)b * out_stride + h * ATT_D + c * DPL + h8 * 8) = o;
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------- paged KV
// The same attention over a PAGED cache with a cache length PER STREAM (include/nsg_attn.h,
// ns_decode_attention_paged).  A stream's rows live in 32-position pages it owns: d_table[b][c] is the device
// address of the page holding stream rows 32c..32c+31 (positions T0 + 32c ...), a page laid out [layer][K|V][H][32]
// [D], so growth only maps new pages (no copy, no second cache) and a finished stream's pages go to the next message
// (slot refill, reference: every message runs its own loop with its own cache, code_base/arithmetic.py:96-122).
//
// With per-stream lengths the row split S of a pair (att_split of its own key count) differs inside a workgroup, so
// the work is cut into TASKS: task (pair j, split w) streams rows s0 + 32w, s0 + 32(w + S), ... exactly as wave w of
// the lockstep kernel does, the 8 waves take the tasks round-robin, every task's partial goes to LDS, and wave j then
// merges pair j's S partials in split order with the lockstep kernel's arithmetic (an S = 1 "merge" is exact: *1,
// +0).  Same rows, same order, same operations: the output bits equal the lockstep kernel's for the same cache
// contents, and still depend on a pair's own key count only (batch-invariant).
//
// Short keys (8-pair workgroups whose pairs are all one wave, a context of at least one whole chunk, no window cutting
// it -- the first 224 steps of every job from a 32-token context): a short path (NSG_ATT_SHORT) with the same
// arithmetic per pair but the context chunk, q and the lengths requested at kernel entry, wave w serving slot w, and
// no loads for rows at or past the new token.  DESIGN §4d, library 0.27.
struct PagedArgs {
    const _Float16* qkv;
    int64_t qkv_stride;
    const uint64_t* table;  // [B][tstride] page addresses (bytes), 0 = no page
    int64_t tstride;
    int max_chunks;         // table entries per stream in use
    int64_t layer_off;      // elements from a page's base to this layer's K block ([layer][K|V][H][32][D])
    int64_t v_off;          // elements from the K block to the V block (H * 32 * D)
    const void* kp;         // shared prefix [H][ph] (positions < T0), fp16 or fp8 like the pages
    const void* vp;
    int64_t ph;
    int T0, B, H;
    const int32_t* lens;    // [B] positions already cached per stream (the new token goes to position lens[b])
    int window;
    const uint32_t* done;
    int64_t done_stride;
    const int32_t* stop;
    _Float16* out;
    int64_t out_stride;
    float scale_log2;
};

#ifndef NSG_ATT_DPP
#define NSG_ATT_DPP 1  // paged kernel: the score sums over a row's LPR lanes and the lane ^ 8 step of the final
                       // row-group merge by DPP moves instead of ds_bpermute
#endif

// x + (x of lane l ^ 1), then + (lane ^ 2), then (LPR = 8) + the other quad's sum -- the xor butterfly's values in
// its order (the third step reads lane 7 - l, whose quad sum equals lane l ^ 4's), as VALU DPP moves instead of
// LDS permutes: the same bits as __shfl_xor's butterfly
template <int LPR>
__device__ __forceinline__ float row_group_sum(float x) {
    static_assert(LPR == 4 || LPR == 8, "rows of 4 or 8 lanes");
    auto dpp = [](float v, auto ctrl) {
        return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v),
                                                                     decltype(ctrl)::value, 0xF, 0xF, false));
    };
    x += dpp(x, std::integral_constant<int, 0xB1>{});  // quad_perm [1,0,3,2]: lane ^ 1
    x += dpp(x, std::integral_constant<int, 0x4E>{});  // quad_perm [2,3,0,1]: lane ^ 2
    if constexpr (LPR == 8) x += dpp(x, std::integral_constant<int, 0x141>{});  // row_half_mirror: lane 7 - l
    return x;
}

__device__ __forceinline__ float row_ror8(float x) {  // the value of lane l ^ 8 (DPP row_ror:8 in a 16-lane row)
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), 0x128, 0xF, 0xF, false));
}

__device__ __forceinline__ uint64_t readlane64(uint64_t v, int lane) {  // lane uniform: the value lands in SGPRs
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, lane);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), lane);
    return ((uint64_t)hi << 32) | lo;
}

#ifndef NSG_ATT_SHORT
#define NSG_ATT_SHORT 1  // paged kernel, 8-pair workgroups: the short-key path (below); 0 = the general path only,
                         // 2 = the short path with the general path's clamped loads in the boundary iterations (A/B)
#endif

// One 32-row iteration of a pair's online softmax: the rows' scores, the running maximum, the rescale and the P.V
// accumulation.  row0 = the position of this lane's row in the first RPI-row slab.  GEN: rows past L0 are masked
// out and row L0 is the new token (knew / vnew, from registers); otherwise every row is a cached one.
// These three helpers are the short-key path's; they restate the task loop's math_chunk, row-group merge and store
// operation for operation (the bits are compared on every stream, tests/test_gpu_paged_short.py).  The task loop
// keeps its own text: routed through the helpers, the P = 1 kernels no longer compiled to the same instructions.
template <class F, bool GEN>
__device__ __forceinline__ void paged_chunk_math(const typename F::Q& q, typename F::Raw (&kr)[F::NI],
                                                 typename F::Raw (&vr)[F::NI], int row0, int L0,
                                                 const typename F::Raw& knew, const typename F::Raw& vnew,
                                                 float scale_log2, float& m, float& l, float (&acc)[F::DPL]) {
    constexpr int DPL = F::DPL, LPR = F::LPR, RPI = F::RPI, NI = F::NI;
    float sc[NI];
    bool valid[NI];
    float mx = m;
#pragma unroll
    for (int u = 0; u < NI; ++u) {
        const int row = row0 + RPI * u;
        valid[u] = GEN ? row <= L0 : true;
        if (GEN && row == L0) {
            kr[u] = knew;
            vr[u] = vnew;
        }
        float sv = F::dot(q, kr[u]);
        if constexpr (NSG_ATT_DPP) {
            sv = row_group_sum<LPR>(sv);
        } else {
#pragma unroll
            for (int off = 1; off < LPR; off <<= 1) sv += __shfl_xor(sv, off);
        }
        sc[u] = sv * scale_log2;
        if (valid[u]) mx = fmaxf(mx, sc[u]);
    }
    const float alpha = exp2f(m - mx);
    l *= alpha;
#pragma unroll
    for (int d = 0; d < DPL; ++d) acc[d] *= alpha;
#pragma unroll
    for (int u = 0; u < NI; ++u) {
        const float p = valid[u] ? exp2f(sc[u] - mx) : 0.0f;
        l += p;
        float v[DPL];
        F::unpack(vr[u], v);
#pragma unroll
        for (int d = 0; d < DPL; ++d) acc[d] = fmaf(p, v[d], acc[d]);
    }
    m = mx;
}

// merge the row groups (lanes c, c + LPR, ... hold the same dims); the lane ^ 8 step as a DPP row_ror:8 (within a
// 16-lane row that IS lane ^ 8; the merge is symmetric in the two lanes, so the same bits), the others through
// ds_bpermute
template <class F>
__device__ __forceinline__ void paged_merge_groups(float& m, float& l, float (&acc)[F::DPL]) {
#pragma unroll
    for (int off = F::LPR; off < 64; off <<= 1) {
        const bool dpp8 = NSG_ATT_DPP && off == 8;
        const float mo = dpp8 ? row_ror8(m) : __shfl_xor(m, off);
        const float lo = dpp8 ? row_ror8(l) : __shfl_xor(l, off);
        const float mn = fmaxf(m, mo);
        const float fa = exp2f(m - mn), fo = exp2f(mo - mn);
        l = l * fa + lo * fo;
#pragma unroll
        for (int d = 0; d < F::DPL; ++d) {
            const float ao = dpp8 ? row_ror8(acc[d]) : __shfl_xor(acc[d], off);
            acc[d] = acc[d] * fa + ao * fo;
        }
        m = mn;
    }
}

// out = acc / l: this lane's DPL dims from o (the pair's output row + the lane's first dim)
template <class F>
__device__ __forceinline__ void paged_store_out(_Float16* o, float l, const float (&acc)[F::DPL]) {
    const float inv = 1.0f / l;
#pragma unroll
    for (int h8 = 0; h8 < F::DPL / 8; ++h8) {
        f16x8 r;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            float tv = acc[h8 * 8 + i] * inv;
            asm volatile("" : "+v"(tv));
            r[i] = (_Float16)tv;
        }
        *(f16x8*)(o + h8 * 8) = r;
    }
}

template <class F, int P>
constexpr int paged_waves_per_eu() {  // NSG_ATT_DB8 fp8: room for the second chunk's registers
    return P == 1 ? 1 : (NSG_ATT_DB8 && std::is_same<F, FmtF8>::value) ? NSG_ATT_DB8_WPE : 4;
}

template <class F, int P>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(paged_waves_per_eu<F, P>()))) void paged_attn_kernel(
    const PagedArgs a) {
    typedef typename F::Elem E;
    typedef typename F::Raw Raw;
    constexpr int DPL = F::DPL, LPR = F::LPR, RPI = F::RPI, NI = F::NI;
    static_assert(RPI * NI == 32, "one iteration = one page's worth of rows");
    constexpr int NT = 8 * P;  // at most 8 splits per pair
    __shared__ float s_m[NT], s_l[NT];
    __shared__ float s_acc[NT][ATT_D];
    __shared__ int s_pi[8][P][4];  // per wave: pair, L0, s0 and first task of each of the workgroup's pairs
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    // Every wave works out the workgroup's pairs itself (lane j < P: pair j's length, skip flags and new-token page;
    // the same few loads in every wave hit the caches) -- no barrier before the streaming starts; the wave keeps
    // them in its own LDS slots, not in registers.
    int pr = -1, pL0 = 0, ps0 = 0, pS = 0, pst = 0;  // status 0 none / skipped, 1 run, 2 poison
    // Short-key path (8 streams of one head per workgroup, context of at least one whole chunk): everything that
    // depends on the workgroup and the lane alone is requested at kernel entry, in one round trip -- the lengths
    // and skip flags first, then the q row of the stream in slot (wave) and the context's first 32 K/V rows of the
    // workgroup's head.  The context rows are shared by the workgroup's 8 waves and by the other workgroups of the
    // head: default cache policy, not non-temporal.  A workgroup that then leaves the short path (a split pair, a
    // window cutting the first chunk) drops these registers; the loads are always legal (T0 >= 32 context rows, a
    // stream index clamped into the batch).
    constexpr bool SHORTP = P == 8 && NSG_ATT_HEAD_MAJOR && NSG_ATT_SHORT;
    const bool ctx32 = SHORTP && a.T0 >= RPI * NI;  // uniform over the launch
    int eL0 = 0, estop = 0;
    uint32_t edone = 0;
    typename F::Q q0 = {};
    Raw ck[NI] = {}, cv[NI] = {};
    if constexpr (SHORTP) {
        {  // every lane asks for the words of slot (lane % P), stream index clamped into the batch: no branch, so
           // nothing waits between these requests and the ones below
            const int bs = min((int)(blockIdx.x / a.H) * P + lane % P, a.B - 1);
            eL0 = a.lens[bs];
            // (absent flags or stops: any readable word, lens[0]; the value is not used)
            edone = *(a.done ? a.done + (int64_t)bs * a.done_stride : (const uint32_t*)a.lens);
            estop = *(a.stop ? a.stop + bs : a.lens);
        }
        if (ctx32) {
            const int h = blockIdx.x % a.H, b = min((int)(blockIdx.x / a.H) * P + wave, a.B - 1);
            const int64_t o = (int64_t)h * a.ph + (lane % LPR) * DPL + (lane / LPR) * ATT_D;  // row (lane / LPR)
            q0 = F::load_q(a.qkv + (int64_t)b * a.qkv_stride + h * ATT_D + (lane % LPR) * DPL);
#pragma unroll
            for (int u = 0; u < NI; ++u) {
                ck[u] = *((const Raw*)((const E*)a.kp + o + RPI * u * ATT_D));
                cv[u] = *((const Raw*)((const E*)a.vp + o + RPI * u * ATT_D));
            }
        }
    }
    if (lane < P) {
        pr = att_pair<P>(blockIdx.x, lane, a.B, a.H);
        if (pr >= 0) {
            const int b = pr / a.H;
            bool skip;
            if constexpr (SHORTP) {
                pL0 = eL0;
                skip = (a.done && (edone & 1u)) || (a.stop && pL0 >= estop);
            } else {
                pL0 = a.lens[b];
                skip = (a.done && (a.done[(int64_t)b * a.done_stride] & 1u)) || (a.stop && pL0 >= a.stop[b]);
            }
            if (!skip) {
                // the new token's stream row: its page must exist (host invariant).  One pair per workgroup (P = 1,
                // small batches): checked here, once; multi-pair workgroups: only the row is checked here and the page
                // by the pair's tasks, one load fewer before their streaming starts (2-3 % at short keys, B = 4,096;
                // at B = 1 the setup check measured 3-4 % faster per token, profiles/r06/c2_attn_setup_ab.txt)
                const int jj = pL0 - a.T0;
                const bool inside = jj >= 0 && (jj >> 5) < a.max_chunks;
                uint64_t pg = inside ? 1u : 0u;
                if constexpr (P == 1) pg = inside ? a.table[(int64_t)b * a.tstride + (jj >> 5)] : 0;
                if (pg == 0 || (P == 1 && (pg & 15u))) {
                    pst = 2;  // no page: poison the output (NaN logits the coder rejects), never write
                } else {
                    pst = 1;
                    const int Lk = pL0 + 1;
                    ps0 = a.window > 0 ? max(0, Lk - a.window) : 0;
                    pS = att_split(Lk - ps0);
                }
            }
        }
    }
    const int g = lane / LPR;  // row within an RPI-row slab
    const int c = lane % LPR;  // DPL-dim slice
    const int C = a.H * ATT_D;
    int pfirst = 0, ntask = 0, multi = 0;  // task index of pair (lane)'s split 0; tasks; any pair split S > 1
#pragma unroll
    for (int k = 0; k < P; ++k) {
        const int sk = __shfl(pS, k);
        pfirst += k < lane ? sk : 0;
        ntask += sk;
        multi |= sk > 1;
    }
    int cut = 0;  // any pair whose window starts past position 0 (its first chunk is not the context's)
    if constexpr (SHORTP) {
#pragma unroll
        for (int k = 0; k < P; ++k) cut |= __shfl(ps0, k);
    }
    if (wave < P && __shfl(pst, wave) == 2) {  // poisoned pair: NaN rows
        const int pair = __shfl(pr, wave);
        a.out[(int64_t)(pair / a.H) * a.out_stride + (pair % a.H) * ATT_D + lane] = (_Float16)__builtin_nanf("");
    }
    if constexpr (SHORTP) {
        // Short-key path: no pair of the workgroup is split (every key count <= NSG_ATT_ROWS1, one wave per pair) and
        // every pair's keys start at position 0, so iteration 0 is the context's first chunk, already in registers.
        // Wave w serves the pair of slot w (a skipped or absent slot's wave retires at once).  The pair's arithmetic
        // is the general path's: rows 0..L0 in order, 32-row iterations, the same online-softmax update, row-group
        // merge and acc / l store -- only addresses, cache policy, load timing and never-used loads differ.
        if (ctx32 && !multi && !cut) {  // uniform over the workgroup
            const int w = __builtin_amdgcn_readfirstlane(wave);
            if (__builtin_amdgcn_readlane(pst, w) != 1) return;  // none, skipped, or poisoned (NaN row written above)
            const int pair = __builtin_amdgcn_readlane(pr, w);
            const int L0 = __builtin_amdgcn_readlane(pL0, w);
            const int T0 = a.T0;
            const int b = pair / a.H, h = pair - b * a.H;
            // the stream's page addresses, chunk i in lane i: chunks 0..cN hold stream rows 0..L0 - T0 (mapped
            // through the new token's chunk: host invariant; cN < max_chunks was checked above, cN <= 7 as the key
            // count is at most NSG_ATT_ROWS1).  One load, second and last round trip before the own rows.
            const int cN = (L0 - T0) >> 5;
            const uint64_t pgv = lane <= cN ? a.table[(int64_t)b * a.tstride + lane] : 0;
            float m = -1e30f, l = 0.0f;
            float acc[DPL];
#pragma unroll
            for (int d = 0; d < DPL; ++d) acc[d] = 0.0f;
            // iteration 0: context rows 0..31 (< T0 <= L0: all valid, none the new token), while the table is in flight
            paged_chunk_math<F, false>(q0, ck, cv, g, L0, ck[0], cv[0], a.scale_log2, m, l, acc);
            const uint64_t apage = readlane64(pgv, cN);  // the new token's page; a missing one poisons the pair
            const bool bad = apage == 0 || (apage & 15u);
            const _Float16* qrow = a.qkv + (int64_t)b * a.qkv_stride + h * ATT_D + c * DPL;
            const int64_t hoff = a.layer_off + (int64_t)h * 32 * ATT_D + c * DPL;  // this layer's K rows of head h
            const E* kpb = (const E*)a.kp + (int64_t)h * a.ph + c * DPL;
            const E* vpb = (const E*)a.vp + (int64_t)h * a.ph + c * DPL;
            Raw knew = {}, vnew = {};
            constexpr bool CLAMP = NSG_ATT_SHORT == 2;  // A/B: rows at or past L0 load a copy of row L0 - 1
            for (int j0 = RPI * NI; j0 <= L0 && !bad; j0 += RPI * NI) {
                const int jj0 = j0 - T0;
                // the chunk of the first stream row the iteration loads; the last one is in ca or ca + 1 (<= 7)
                const int ca = max(CLAMP ? min(jj0, L0 - 1 - T0) : jj0, 0) >> 5;
                const E* pa = (const E*)readlane64(pgv, ca) + hoff;
                const E* pb = (const E*)readlane64(pgv, ca + 1) + hoff;
                if (jj0 >= 0 && j0 + RPI * NI <= L0) {  // interior: stream rows < L0 only
#pragma unroll
                    for (int u = 0; u < NI; ++u) {
                        const int jj = jj0 + RPI * u + g;
                        const E* ka = ((jj >> 5) == ca ? pa : pb) + (int64_t)(jj & 31) * ATT_D;
                        ck[u] = att_load((const Raw*)ka);
                        cv[u] = att_load((const Raw*)(ka + a.v_off));
                    }
                    paged_chunk_math<F, false>(q0, ck, cv, j0 + g, L0, knew, vnew, a.scale_log2, m, l, acc);
                    continue;
                }
                // Boundary iteration (context rows past the first chunk, the new token, rows past it).  Only rows
                // < L0 are loaded: row L0 is the new token, from the qkv row (requested here, with the last chunk, so
                // it holds no registers during the stream), and a row past L0 keeps the bit pattern 0 = +0.0 in
                // either format.  The general path feeds such a row a copy of row L0 - 1 instead; the bits cannot
                // differ: the row is masked (valid = false), so its score never reaches the maximum, p = 0,
                // l + 0 = l, and acc -- which starts at +0 and, sums under round-to-nearest never giving -0 unless
                // both terms are -0, is never -0 -- takes fmaf(0, finite, acc) = acc for either value.  No register
                // reaches the arithmetic uninitialised.
                const bool lastit = j0 + RPI * NI > L0;
                if (lastit) {
                    knew = F::from_qkv(qrow + C);
                    vnew = F::from_qkv(qrow + 2 * C);
                }
#pragma unroll
                for (int u = 0; u < NI; ++u) {
                    const int row = CLAMP ? min(j0 + RPI * u + g, L0 - 1) : j0 + RPI * u + g;
                    ck[u] = Raw{};
                    cv[u] = Raw{};
                    if (row < T0) {  // shared by the head's workgroups: default policy
                        ck[u] = *(const Raw*)(kpb + (int64_t)row * ATT_D);
                        cv[u] = *(const Raw*)(vpb + (int64_t)row * ATT_D);
                    } else if (row < L0) {
                        const int jj = row - T0;
                        const E* ka = ((jj >> 5) == ca ? pa : pb) + (int64_t)(jj & 31) * ATT_D;
                        ck[u] = att_load((const Raw*)ka);
                        cv[u] = att_load((const Raw*)(ka + a.v_off));
                    }
                }
                paged_chunk_math<F, true>(q0, ck, cv, j0 + g, L0, knew, vnew, a.scale_log2, m, l, acc);
                if (lastit && g == 0) {  // KV append of the new token (position L0)
                    E* kd = (E*)apage + hoff + (int64_t)((L0 - T0) & 31) * ATT_D;
                    *(Raw*)kd = knew;
                    *(Raw*)(kd + a.v_off) = vnew;
                }
            }
            paged_merge_groups<F>(m, l, acc);
            if (bad) {
                l = __builtin_nanf("");
#pragma unroll
                for (int d = 0; d < DPL; ++d) acc[d] = __builtin_nanf("");
            }
            if (g == 0) paged_store_out<F>(a.out + (int64_t)b * a.out_stride + h * ATT_D + c * DPL, l, acc);
            return;
        }
    }
    if (lane < P) {
        s_pi[wave][lane][0] = pr;
        s_pi[wave][lane][1] = pL0;
        s_pi[wave][lane][2] = ps0;
        s_pi[wave][lane][3] = pfirst;
    }
    const int myS = wave < P ? __shfl(pS, wave) : 0;  // the merge phase's pair (wave) split
    __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0): the wave's own LDS slots are written before they are read
    __builtin_amdgcn_wave_barrier();
    for (int t = wave; t < ntask; t += 8) {  // wave-uniform
        int j = 0;
#pragma unroll
        for (int k = 1; k < P; ++k)
            if (t >= s_pi[wave][k][3]) j = k;  // the last pair whose first task is <= t (pairs without tasks share
                                               // the next one's first task and are passed over)
        const int pair = __builtin_amdgcn_readfirstlane(s_pi[wave][j][0]);
        const int L0 = __builtin_amdgcn_readfirstlane(s_pi[wave][j][1]);
        const int s0 = __builtin_amdgcn_readfirstlane(s_pi[wave][j][2]);
        const int wv = t - __builtin_amdgcn_readfirstlane(s_pi[wave][j][3]);
        const int S = att_split(L0 + 1 - s0);
        const int T0 = a.T0;
        const int Lk = L0 + 1;
        const int last_cached = L0 > 0 ? L0 - 1 : 0;
        const int b = pair / a.H, h = pair - b * a.H;
        const uint64_t* trow = a.table + (int64_t)b * a.tstride;
        const _Float16* qrow = a.qkv + (int64_t)b * a.qkv_stride + h * ATT_D + c * DPL;
        const typename F::Q q = F::load_q(qrow);
        const Raw knew = F::from_qkv(qrow + C);
        const Raw vnew = F::from_qkv(qrow + 2 * C);
        const int64_t hoff = a.layer_off + (int64_t)h * 32 * ATT_D + c * DPL;  // this layer's K rows of head h
        auto kaddr = [&](uint64_t page, int jj) -> E* { return (E*)page + hoff + (int64_t)(jj & 31) * ATT_D; };
        const E* kpb = (const E*)a.kp + (int64_t)h * a.ph + c * DPL;
        const E* vpb = (const E*)a.vp + (int64_t)h * a.ph + c * DPL;
        if constexpr (P == 1) {
            if (g == 0 && wv == 0) {  // KV append of the new token (position L0, page checked in the setup)
                E* kd = kaddr(trow[(L0 - T0) >> 5], L0 - T0);
                *(Raw*)kd = knew;
                *(Raw*)(kd + a.v_off) = vnew;
            }
        }
        float m = -1e30f, l = 0.0f;
        float acc[DPL];
#pragma unroll
        for (int d = 0; d < DPL; ++d) acc[d] = 0.0f;
        const int step = S * RPI * NI;
        const int jbeg = s0 + wv * RPI * NI;
        // page addresses of 64 iterations at a time, one per lane (lane i: iteration kbase + i; the first and the
        // last page of the stream rows it reads -- rows past the cache are clamped to the last cached one), read
        // back with readlane: no dependent table load inside the stream
        const int hi_row = last_cached - T0;  // the last stream row an iteration reads (< 0: prefix rows only)
        int kbase = -64;
        uint64_t pgA = 0, pgB = 0;
        auto pages_of = [&](int k, uint64_t& pa, uint64_t& pb) {
            if (k - kbase >= 64) {
                kbase = k;
                const int jj = jbeg + (k + lane) * step - T0;
                // rows read: [jj, jj + 31] clamped to the last cached row (as load_chunk clamps them); stream rows
                // only (< 0: the shared prefix); beyond the job's iterations the lane loads nothing
                const int lo = max(min(jj, hi_row), 0), hi = min(jj + RPI * NI - 1, hi_row);
                const bool any = hi >= 0 && jj <= L0 - T0;
                pgA = any ? trow[lo >> 5] : 0;
                pgB = any && (hi >> 5) != (lo >> 5) ? trow[hi >> 5] : pgA;
            }
            pa = readlane64(pgA, k - kbase);
            pb = readlane64(pgB, k - kbase);
        };
        // multi-pair workgroups: the new token's page -- a missing one (host invariant broken) poisons the pair: every
        // one of its tasks reads the same entry, writes nothing and hands NaN on (S = 1: the output row; S > 1: the
        // partials, which the merge turns into NaN).  The first iterations' page addresses are requested before it,
        // so both table reads are in flight together (the prefetch reads entries of cached rows only).
        bool bad = false;
        if constexpr (P > 1) {
            {
                uint64_t pa0, pb0;
                pages_of(0, pa0, pb0);
            }
            const uint64_t apage = trow[(L0 - T0) >> 5];
            bad = apage == 0 || (apage & 15u);
            if (g == 0 && wv == 0 && !bad) {  // KV append of the new token (position L0)
                E* kd = kaddr(apage, L0 - T0);
                *(Raw*)kd = knew;
                *(Raw*)(kd + a.v_off) = vnew;
            }
        }
        const int Lend = bad ? 0 : Lk;  // the streaming loops run while j0 < Lend
        // one iteration = RPI*NI = 32 consecutive rows from j0; GENERAL handles the prefix boundary, the clamp past
        // the cache and the new token; an interior run (stream rows < L0 only) spans at most two pages
        auto load_chunk = [&](int j0, int k, auto general, Raw (&kr)[NI], Raw (&vr)[NI]) {
            constexpr bool GEN = decltype(general)::value;
            uint64_t pa, pb;
            pages_of(k, pa, pb);
            if constexpr (GEN) {
                const int ca = max(min(j0 - T0, hi_row), 0) >> 5;  // the chunk of the first stream row read (pa)
#pragma unroll
                for (int u = 0; u < NI; ++u) {
                    const int row = min(j0 + RPI * u + g, last_cached);
                    if (row < T0) {
                        kr[u] = att_load((const Raw*)(kpb + (int64_t)row * ATT_D));
                        vr[u] = att_load((const Raw*)(vpb + (int64_t)row * ATT_D));
                    } else {
                        const int jj = row - T0;
                        const E* ka = kaddr((jj >> 5) == ca ? pa : pb, jj);
                        kr[u] = att_load((const Raw*)ka);
                        vr[u] = att_load((const Raw*)(ka + a.v_off));
                    }
                }
            } else {
                const int jj0 = j0 - T0;
                const int ca = jj0 >> 5;
#pragma unroll
                for (int u = 0; u < NI; ++u) {
                    const int jj = jj0 + RPI * u + g;
                    const E* ka = kaddr((jj >> 5) == ca ? pa : pb, jj);
                    kr[u] = att_load((const Raw*)ka);
                    vr[u] = att_load((const Raw*)(ka + a.v_off));
                }
            }
        };
        auto math_chunk = [&](int j0, auto general, Raw (&kr)[NI], Raw (&vr)[NI]) {
            constexpr bool GEN = decltype(general)::value;
            float sc[NI];
            bool valid[NI];
            float mx = m;
#pragma unroll
            for (int u = 0; u < NI; ++u) {
                const int row = j0 + RPI * u + g;
                valid[u] = GEN ? row < Lk : true;
                if (GEN && row == L0) {
                    kr[u] = knew;
                    vr[u] = vnew;
                }
                float sv = F::dot(q, kr[u]);
                if constexpr (NSG_ATT_DPP) {
                    sv = row_group_sum<LPR>(sv);
                } else {
#pragma unroll
                    for (int off = 1; off < LPR; off <<= 1) sv += __shfl_xor(sv, off);
                }
                sc[u] = sv * a.scale_log2;
                if (valid[u]) mx = fmaxf(mx, sc[u]);
            }
            const float alpha = exp2f(m - mx);
            l *= alpha;
#pragma unroll
            for (int d = 0; d < DPL; ++d) acc[d] *= alpha;
#pragma unroll
            for (int u = 0; u < NI; ++u) {
                const float p = valid[u] ? exp2f(sc[u] - mx) : 0.0f;
                l += p;
                float v[DPL];
                F::unpack(vr[u], v);
#pragma unroll
                for (int d = 0; d < DPL; ++d) acc[d] = fmaf(p, v[d], acc[d]);
            }
            m = mx;
        };
        auto interior = [&](int j0) { return j0 >= T0 && j0 + RPI * NI <= L0; };
        Raw kr[NI], vr[NI];
        if constexpr (P > 1 && !(NSG_ATT_DB8 && std::is_same<F, FmtF8>::value)) {
            int k = 0;
            for (int j0 = jbeg; j0 < Lend; j0 += step, ++k) {
                if (interior(j0)) {
                    load_chunk(j0, k, std::false_type{}, kr, vr);
                    math_chunk(j0, std::false_type{}, kr, vr);
                } else {
                    load_chunk(j0, k, std::true_type{}, kr, vr);
                    math_chunk(j0, std::true_type{}, kr, vr);
                }
            }
        } else {  // one pair per workgroup (small batches; NSG_ATT_DB8: fp8 always): register double buffer, as the
                  // lockstep kernel
            Raw kn[NI], vn[NI];
            int j0 = jbeg, k = 0;
            if (j0 < Lend) {
                if (interior(j0))
                    load_chunk(j0, 0, std::false_type{}, kr, vr);
                else
                    load_chunk(j0, 0, std::true_type{}, kr, vr);
            }
            for (; j0 < Lend; j0 += step, ++k) {
                const int j1 = j0 + step;
                if (j1 < Lend) {
                    if (interior(j1))
                        load_chunk(j1, k + 1, std::false_type{}, kn, vn);
                    else
                        load_chunk(j1, k + 1, std::true_type{}, kn, vn);
                }
                if (interior(j0))
                    math_chunk(j0, std::false_type{}, kr, vr);
                else
                    math_chunk(j0, std::true_type{}, kr, vr);
#pragma unroll
                for (int u = 0; u < NI; ++u) {
                    kr[u] = kn[u];
                    vr[u] = vn[u];
                }
            }
        }
        // merge the row groups (lanes c, c + LPR, ... hold the same dims); the lane ^ 8 step as a DPP row_ror:8
        // (within a 16-lane row that IS lane ^ 8; the merge is symmetric in the two lanes, so the same bits), the
        // others through ds_bpermute
#pragma unroll
        for (int off = LPR; off < 64; off <<= 1) {
            const bool dpp8 = NSG_ATT_DPP && off == 8;
            const float mo = dpp8 ? row_ror8(m) : __shfl_xor(m, off);
            const float lo = dpp8 ? row_ror8(l) : __shfl_xor(l, off);
            const float mn = fmaxf(m, mo);
            const float fa = exp2f(m - mn), fo = exp2f(mo - mn);
            l = l * fa + lo * fo;
#pragma unroll
            for (int d = 0; d < DPL; ++d) {
                const float ao = dpp8 ? row_ror8(acc[d]) : __shfl_xor(acc[d], off);
                acc[d] = acc[d] * fa + ao * fo;
            }
            m = mn;
        }
        if (bad) {
            m = l = __builtin_nanf("");
#pragma unroll
            for (int d = 0; d < DPL; ++d) acc[d] = __builtin_nanf("");
        }
        if (S == 1) {  // the whole pair in this wave: out = acc / l, as the lockstep kernel (a 1-way merge is exact)
            if (g == 0) {
                const float inv = 1.0f / l;
#pragma unroll
                for (int h8 = 0; h8 < DPL / 8; ++h8) {
                    f16x8 o;
#pragma unroll
                    for (int i = 0; i < 8; ++i) {
                        float tv = acc[h8 * 8 + i] * inv;
                        asm volatile("" : "+v"(tv));
                        o[i] = (_Float16)tv;
                    }
                    *(f16x8*)(a.out + (int64_t)b * a.out_stride + h * ATT_D + c * DPL + h8 * 8) = o;
                }
            }
        } else if (g == 0) {
#pragma unroll
            for (int d = 0; d < DPL; ++d) s_acc[t][c * DPL + d] = acc[d];
            if (c == 0) {
                s_m[t] = m;
                s_l[t] = l;
            }
        }
    }
    if (!multi) return;  // uniform: no pair was split over waves
    __syncthreads();
    // pair (wave) split over S > 1 waves: merge the S partials in split order, as the lockstep kernel does
    if (wave >= P || lane >= LPR) return;
    const int S = myS;
    if (S <= 1) return;
    const int w0 = s_pi[wave][wave][3];
    const int pair = s_pi[wave][wave][0];
    const int b = pair / a.H, h = pair - b * a.H;
    float mt = s_m[w0];
    for (int w = 1; w < S; ++w) mt = fmaxf(mt, s_m[w0 + w]);
    float l = 0.0f;
    float acc[DPL];
#pragma unroll
    for (int d = 0; d < DPL; ++d) acc[d] = 0.0f;
    for (int w = 0; w < S; ++w) {
        const float f = exp2f(s_m[w0 + w] - mt);
        l += s_l[w0 + w] * f;
#pragma unroll
        for (int d = 0; d < DPL; ++d) acc[d] += s_acc[w0 + w][lane * DPL + d] * f;
    }
    const float inv = 1.0f / l;
#pragma unroll
    for (int h8 = 0; h8 < DPL / 8; ++h8) {
        f16x8 o;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            float tv = acc[h8 * 8 + i] * inv;
            asm volatile("" : "+v"(tv));
            o[i] = (_Float16)tv;
        }
        *(f16x8*)(a.out + (int64_t)b * a.out_stride + h * ATT_D + lane * DPL + h8 * 8) = o;
    }
}

// ------------------------------------------------------------------------------------ paged KV, C queries a stream
// ns_decode_attention_paged_chunk (include/nsg_attn.h): stream b's next n <= C tokens in one launch, each query's
// output the bits of the one-token kernel at that query's own key count.  Workgroup = one (stream, head) pair.
//
// The one-token kernel cuts query i (key count Lk = L + i + 1) into S = att_split(Lk) tasks, task w streaming the
// 32-row chunks w, w + S, ... in order.  Queries of one launch with the same S have the same chunk sequences, so a
// GROUP (S, w, query range) loads each chunk once and applies it to every query of the range whose key count reaches
// it, one (m, l, acc) state per query in registers, CT queries at a time.  A chunk of at most 16 queries crosses at
// most one of att_split's thresholds, so there are S groups, or S_lo + S_hi (at most 12) when it crosses one; the
// waves take the groups round-robin.  Per query the operations are paged_chunk_math's, in the one-token kernel's row
// order, with that kernel's choice between the interior and the general form; then paged_merge_groups, and either
// paged_store_out (S = 1) or partials through LDS merged in split order with the one-token kernel's arithmetic.
//
// The n new rows are converted once (F::from_qkv), stored to the pages and kept in LDS; a chunk takes rows >= L from
// there (the bytes an earlier one-token call would have stored and a later one loaded).  A row past a query's own
// position is fed as the bit pattern 0 and masked, as the one-token kernel's short path feeds it (see there why the
// bits cannot differ from the clamped copy the general path feeds).  Pages are only read below L and only written at
// L .. L + n - 1, so no wave reads what another writes.
constexpr int ATT_CHUNK_MAX = 16;

template <class F, int CT, int NW>
__global__ __launch_bounds__(64 * NW) void paged_attn_chunk_kernel(const PagedArgs a, const int C,
                                                                   const int32_t* __restrict__ count) {
    typedef typename F::Elem E;
    typedef typename F::Raw Raw;
    constexpr int DPL = F::DPL, LPR = F::LPR, RPI = F::RPI, NI = F::NI;
    static_assert(RPI * NI == 32, "one iteration = one page's worth of rows");
    __shared__ float s_m[ATT_CHUNK_MAX][8], s_l[ATT_CHUNK_MAX][8];
    __shared__ float s_acc[ATT_CHUNK_MAX][8][ATT_D];
    __shared__ Raw s_kn[ATT_CHUNK_MAX][LPR], s_vn[ATT_CHUNK_MAX][LPR];  // the new rows, as the pages hold them
    __shared__ __attribute__((aligned(16))) _Float16 s_q[ATT_CHUNK_MAX][ATT_D];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int b = blockIdx.x / a.H, h = blockIdx.x - b * a.H;
    const int n = min(count[b], C);
    if (n <= 0) return;  // uniform over the workgroup: the stream is left untouched
    const int L = a.lens[b];
    const int T0 = a.T0;
    const int HD = a.H * ATT_D;
    const uint64_t* trow = a.table + (int64_t)b * a.tstride;
    // the pages of the new rows (stream rows jn .. jn + n - 1: at most two chunks) must exist
    const int64_t jn = (int64_t)L - T0;
    bool bad = jn < 0 || ((jn + n - 1) >> 5) >= a.max_chunks;
    uint64_t pn0 = 0, pn1 = 0;
    if (!bad) {
        pn0 = trow[jn >> 5];
        pn1 = trow[(jn + n - 1) >> 5];
        bad = pn0 == 0 || (pn0 & 15u) || pn1 == 0 || (pn1 & 15u);
    }
    if (bad) {  // uniform: NaN rows (the coder rejects them), no page byte written
        if (tid < ATT_D)
            for (int i = 0; i < n; ++i)
                a.out[((int64_t)b * C + i) * a.out_stride + h * ATT_D + tid] = (_Float16)__builtin_nanf("");
        return;
    }
    const int64_t hbase = a.layer_off + (int64_t)h * 32 * ATT_D;  // this layer's K rows of head h in a page
    if (tid < n * LPR) {  // convert, append and keep the new rows; q rows to LDS
        const int i = tid / LPR, cc = tid % LPR;
        const _Float16* qrow = a.qkv + ((int64_t)b * C + i) * a.qkv_stride + h * ATT_D + cc * DPL;
        const Raw kn = F::from_qkv(qrow + HD), vn = F::from_qkv(qrow + 2 * HD);
        s_kn[i][cc] = kn;
        s_vn[i][cc] = vn;
#pragma unroll
        for (int h8 = 0; h8 < DPL / 8; ++h8) *(f16x8*)&s_q[i][cc * DPL + h8 * 8] = *(const f16x8*)(qrow + h8 * 8);
        const int64_t jj = jn + i;
        E* kd = (E*)((jj >> 5) == (jn >> 5) ? pn0 : pn1) + hbase + (jj & 31) * ATT_D + cc * DPL;
        *(Raw*)kd = kn;
        *(Raw*)(kd + a.v_off) = vn;
    }
    __syncthreads();
    const int g = lane / LPR;  // row within an RPI-row slab
    const int c = lane % LPR;  // DPL-dim slice
    // groups: queries [0, ib) split S_lo ways, queries [ib, n) S_hi ways (ib = n when no threshold is crossed)
    const int S_lo = att_split(L + 1), S_hi = att_split(L + n);
    const int ib = S_lo == S_hi ? n : S_lo * NSG_ATT_ROWS1 - L;  // first query whose key count exceeds the threshold
    const int ngroups = S_lo == S_hi ? S_lo : S_lo + S_hi;
    const int cl = L > T0 ? (L - 1 - T0) >> 5 : -1;  // the last chunk holding a cached stream row (< max_chunks)
    const E* kpb = (const E*)a.kp + (int64_t)h * a.ph + c * DPL;
    const E* vpb = (const E*)a.vp + (int64_t)h * a.ph + c * DPL;
    const int64_t hoff = hbase + c * DPL;
    for (int gi = wave; gi < ngroups; gi += NW) {  // wave-uniform
        const bool lo = gi < S_lo;
        const int S = lo ? S_lo : S_hi, w = lo ? gi : gi - S_lo;
        const int i_beg = lo ? 0 : ib, i_end = lo ? ib : n;
        for (int q0 = i_beg; q0 < i_end; q0 += CT) {
            const int nq = min(CT, i_end - q0);
            float m[CT], l[CT], acc[CT][DPL];
#pragma unroll
            for (int ii = 0; ii < CT; ++ii) {
                m[ii] = -1e30f;
                l[ii] = 0.0f;
#pragma unroll
                for (int d = 0; d < DPL; ++d) acc[ii][d] = 0.0f;
            }
            bool hole = false;  // a cached row's table entry is zero or misaligned: nothing read there, NaN rows
            int pbase = -1;     // lane i holds table entry pbase + i (entries of cached rows only)
            uint64_t pgv = 0;
            const int Lmax = L + q0 + nq;  // the key count of the batch's last query
            for (int j0 = w * RPI * NI; j0 < Lmax; j0 += S * RPI * NI) {
                Raw kr[NI], vr[NI];
                const int ca = max(j0 - T0, 0) >> 5;  // the chunk of the first stream row of the iteration
                uint64_t pa = 0, pb = 0;
                if (ca <= cl) {
                    if (pbase < 0 || ca + 1 >= pbase + 64) {
                        pbase = ca;
                        pgv = ca + lane <= cl ? trow[ca + lane] : 0;
                    }
                    pa = readlane64(pgv, ca - pbase);
                    pb = readlane64(pgv, ca + 1 - pbase);
                    if (pa & 15u) pa = 0;
                    if (pb & 15u) pb = 0;
                }
                if (j0 >= T0 && j0 + RPI * NI <= L && pa != 0 && (pb != 0 || ((j0 - T0) & 31) == 0)) {
                    const int jj0 = j0 - T0;  // cached stream rows only, in at most two pages
#pragma unroll
                    for (int u = 0; u < NI; ++u) {
                        const int jj = jj0 + RPI * u + g;
                        const E* ka = (const E*)((jj >> 5) == ca ? pa : pb) + hoff + (int64_t)(jj & 31) * ATT_D;
                        kr[u] = att_load((const Raw*)ka);
                        vr[u] = att_load((const Raw*)(ka + a.v_off));
                    }
                } else {
#pragma unroll
                    for (int u = 0; u < NI; ++u) {
                        const int row = j0 + RPI * u + g;
                        kr[u] = Raw{};
                        vr[u] = Raw{};
                        if (row < T0) {
                            kr[u] = *(const Raw*)(kpb + (int64_t)row * ATT_D);
                            vr[u] = *(const Raw*)(vpb + (int64_t)row * ATT_D);
                        } else if (row < L) {
                            const int jj = row - T0;
                            const uint64_t pg = (jj >> 5) == ca ? pa : pb;
                            if (pg != 0) {
                                const E* ka = (const E*)pg + hoff + (int64_t)(jj & 31) * ATT_D;
                                kr[u] = att_load((const Raw*)ka);
                                vr[u] = att_load((const Raw*)(ka + a.v_off));
                            } else {
                                hole = true;
                            }
                        } else if (row < L + n) {
                            kr[u] = s_kn[row - L][c];
                            vr[u] = s_vn[row - L][c];
                        }
                    }
                }
#pragma unroll
                for (int ii = 0; ii < CT; ++ii) {
                    const int L0 = L + q0 + ii;  // query q0 + ii attends to positions 0 .. L0
                    if (ii >= nq || j0 > L0) continue;  // uniform
                    const typename F::Q q = F::load_q(&s_q[q0 + ii][c * DPL]);
                    if (j0 >= T0 && j0 + RPI * NI <= L0) {  // the one-token kernel's interior iteration
                        paged_chunk_math<F, false>(q, kr, vr, j0 + g, L0, kr[0], vr[0], a.scale_log2, m[ii], l[ii],
                                                   acc[ii]);
                    } else {
                        Raw kq[NI], vq[NI];
#pragma unroll
                        for (int u = 0; u < NI; ++u) {
                            const bool own = j0 + RPI * u + g <= L0;
                            kq[u] = own ? kr[u] : Raw{};
                            vq[u] = own ? vr[u] : Raw{};
                        }
                        const Raw knew = s_kn[q0 + ii][c], vnew = s_vn[q0 + ii][c];
                        paged_chunk_math<F, true>(q, kq, vq, j0 + g, L0, knew, vnew, a.scale_log2, m[ii], l[ii],
                                                  acc[ii]);
                    }
                }
            }
            hole = __any(hole);
#pragma unroll
            for (int ii = 0; ii < CT; ++ii) {
                if (ii >= nq) continue;  // uniform
                const int i = q0 + ii;
                paged_merge_groups<F>(m[ii], l[ii], acc[ii]);
                if (hole) {
                    m[ii] = l[ii] = __builtin_nanf("");
#pragma unroll
                    for (int d = 0; d < DPL; ++d) acc[ii][d] = __builtin_nanf("");
                }
                if (S == 1) {  // the whole query in this wave
                    if (g == 0)
                        paged_store_out<F>(a.out + ((int64_t)b * C + i) * a.out_stride + h * ATT_D + c * DPL, l[ii],
                                           acc[ii]);
                } else if (g == 0) {
#pragma unroll
                    for (int d = 0; d < DPL; ++d) s_acc[i][w][c * DPL + d] = acc[ii][d];
                    if (c == 0) {
                        s_m[i][w] = m[ii];
                        s_l[i][w] = l[ii];
                    }
                }
            }
        }
    }
    if (S_hi <= 1) return;  // uniform: no query was split over waves
    __syncthreads();
    // queries split over S > 1 tasks: merge the S partials in split order, as the one-token kernel does
    if (lane >= LPR) return;
    for (int i = wave; i < n; i += NW) {
        const int S = att_split(L + i + 1);
        if (S <= 1) continue;
        float mt = s_m[i][0];
        for (int w = 1; w < S; ++w) mt = fmaxf(mt, s_m[i][w]);
        float l = 0.0f;
        float acc[DPL];
#pragma unroll
        for (int d = 0; d < DPL; ++d) acc[d] = 0.0f;
        for (int w = 0; w < S; ++w) {
            const float f = exp2f(s_m[i][w] - mt);
            l += s_l[i][w] * f;
#pragma unroll
            for (int d = 0; d < DPL; ++d) acc[d] += s_acc[i][w][lane * DPL + d] * f;
        }
        const float inv = 1.0f / l;
#pragma unroll
        for (int h8 = 0; h8 < DPL / 8; ++h8) {
            f16x8 o;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                float tv = acc[h8 * 8 + k] * inv;
                asm volatile("" : "+v"(tv));
                o[k] = (_Float16)tv;
            }
            *(f16x8*)(a.out + ((int64_t)b * C + i) * a.out_stride + h * ATT_D + lane * DPL + h8 * 8) = o;
        }
    }
}

// fp16 -> fp8 (e4m3fn) with the same saturating round-to-nearest-even conversion as the kernel's KV append
__global__ void quantize_fp8_kernel(const _Float16* __restrict__ src, uint32_t* __restrict__ dst, int64_t n4) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n4) return;
    const _Float16* s4 = src + 4 * i;
    dst[i] = pack4_fp8((float)s4[0], (float)s4[1], (float)s4[2], (float)s4[3]);
}

// ------------------------------------------------------------------------------------------ causal sequences
// softmax(q k^T / sqrt(D) + causal mask) v over B sequences of T tokens at once: the shared-context prefill
// (code_base/arithmetic.py:115-122, first call), the guard's scoring forward (metrics/lm_scorer.py:121-131) and
// the max_context window forward of the src provider (lm/arithmetic.py:45-74).  Flash attention on the
// v_mfma_f32_16x16x32_f16 matrix cores: a workgroup of 4 waves owns 64 queries of one (sequence, head), each wave
// 16; key blocks of 64 are staged in LDS (K as [key][d], V transposed as [d][key], 16-byte chunks XOR-swizzled
// by (row >> 1) & 7 so every ds_read_b128 of a 16-lane group hits distinct banks); per block S = K Q^T (lane
// (r, c) holds query r's scores of keys 4c..4c+3 of each 16-key tile), an online softmax in fp32 (exp2, log2 e
// folded into the scale), P staged through LDS as fp16, O += V^T P (lane holds dims 4c..4c+3 of each 16-dim tile
// of query r).  A query's result depends only on its own sequence (fixed block order 0..its block, fixed MFMA
// chains), never on B or on the other queries of the tile: batch-invariant like the decode step.
typedef _Float16 sq_f16x4 __attribute__((ext_vector_type(4)));
typedef float sq_f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ sq_f32x4 sq_mfma(f16x8 a, f16x8 b, sq_f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ int sq_swz(int row) { return (row >> 1) & 7; }
__device__ __forceinline__ _Float16 sq_h(float v) {  // fp32 pinned before the conversion (no fused rounding)
    asm volatile("" : "+v"(v));
    return (_Float16)v;
}

// Where the ragged form (ns_seq_attention_ragged) keeps a sequence's K/V: stream row r of the sequence goes to page
// table[r / 32] (the sequence's table row), at layer_off + [K|V][H][32][D] as ns_decode_attention_paged reads it.
struct SeqStore {
    const uint64_t* table;  // the sequence's table row (entries 0..max_chunks-1; 0 = no page: rows not stored)
    int max_chunks;
    int64_t layer_off;      // elements from a page's address to this layer's K block
    int64_t v_off;          // elements from the K block to the V block (H * 32 * D)
    int past;               // PAST form only: absolute rows 0..past-1 of the sequence are already in its pages
};

// One workgroup: the 64 queries of block qb of ONE sequence of T rows, head columns at `base` (the sequence's first
// qkv row + h * D), output rows at `obase` (its first output row + h * D).  Every row index is clamped into the
// sequence (min(row, T - 1)): no row outside [0, T) of the sequence is read.  STORE 0: attention only (the bits
// of ns_seq_attention); 1 / 2: the workgroup also writes the 64 keys it stages for its own diagonal block
// (kb == qb, rows < T) to the sequence's pages, fp16 copies / fp8 with the decode append's conversion (pack4_fp8
// over 4 consecutive dims, as FmtF8::from_qkv) -- every (sequence, head, block) exactly once, from the registers
// the staging holds anyway.
// PAST (ns_seq_attention_ragged_past, fp16 pages): the sequence's first ps.past rows (a multiple of 64, every entry of
// table[0 .. past/32) checked by the caller) are in its pages and `base` / `obase` are its row ps.past; T and qb stay
// ABSOLUTE (T = past + new rows, qb >= past/64).  Key blocks kb < past/64 are staged from pages 2kb and 2kb+1 -- the
// bit copies an earlier launch stored there -- the others from the packed rows as ever; everything after the staging
// is the one body, so a split at a multiple of 64 changes no bit of the output or of the stored rows.
template <int STORE, bool PAST = false>
__device__ __forceinline__ void seq_attn_block(const _Float16* __restrict__ base, int64_t qkv_stride,
                                               _Float16* __restrict__ obase, int64_t out_stride, int T, int qb, int h,
                                               int C, float scale_log2, const SeqStore& ps) {
    __shared__ __attribute__((aligned(16))) _Float16 sK[64 * ATT_D];
    __shared__ __attribute__((aligned(16))) _Float16 sVt[ATT_D * 64];
    __shared__ __attribute__((aligned(16))) _Float16 sP[4][16 * 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = lane & 15, c = lane >> 4;
    const int tq = qb * 64 + wave * 16 + r;  // this lane's query (padding rows past T are computed, not stored)
    const int past = PAST ? ps.past : 0;     // packed row = absolute row - past
    f16x8 qf[2];
#pragma unroll
    for (int dc = 0; dc < 2; ++dc)
        qf[dc] = *(const f16x8*)(base + (int64_t)(min(tq, T - 1) - past) * qkv_stride + dc * 32 + c * 8);
    sq_f32x4 o[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) o[dt] = sq_f32x4{0.f, 0.f, 0.f, 0.f};
    float m = -1e30f, l = 0.0f;
    _Float16* Pw = sP[wave];
    for (int kb = 0; kb <= qb; ++kb) {
        __syncthreads();  // the previous block's K / V reads are done
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int id = (int)threadIdx.x + 256 * u;
            const int key = id >> 3, ch = id & 7;
            f16x8 kv, vv;
            if (PAST && kb * 64 < past) {  // (uniform) a full block of stored rows: one 16-byte load per (key, chunk)
                const _Float16* src = (const _Float16*)ps.table[2 * kb + (key >> 5)] + ps.layer_off +
                                      (int64_t)h * 32 * ATT_D + (int64_t)(key & 31) * ATT_D + ch * 8;
                kv = *(const f16x8*)src;
                vv = *(const f16x8*)(src + ps.v_off);
            } else {
                const _Float16* src = base + (int64_t)(min(kb * 64 + key, T - 1) - past) * qkv_stride + ch * 8;
                kv = *(const f16x8*)(src + C);
                vv = *(const f16x8*)(src + 2 * C);
            }
            *(f16x8*)(sK + key * 64 + ((ch ^ sq_swz(key)) * 8)) = kv;
            if constexpr (STORE != 0) {
                const int row = kb * 64 + key;  // uniform test first: only the diagonal block's workgroup stores
                if (kb == qb && row < T && (row >> 5) < ps.max_chunks) {
                    const uint64_t pg = ps.table[row >> 5];
                    if (pg != 0 && !(pg & 15u)) {
                        const int64_t e = ps.layer_off + (int64_t)h * 32 * ATT_D + (int64_t)(row & 31) * ATT_D + ch * 8;
                        if constexpr (STORE == 1) {
                            _Float16* kd = (_Float16*)pg + e;
                            *(f16x8*)kd = kv;
                            *(f16x8*)(kd + ps.v_off) = vv;
                        } else {
                            uint8_t* kd = (uint8_t*)pg + e;
                            uint2 k8, v8;
                            k8.x = pack4_fp8((float)kv[0], (float)kv[1], (float)kv[2], (float)kv[3]);
                            k8.y = pack4_fp8((float)kv[4], (float)kv[5], (float)kv[6], (float)kv[7]);
                            v8.x = pack4_fp8((float)vv[0], (float)vv[1], (float)vv[2], (float)vv[3]);
                            v8.y = pack4_fp8((float)vv[4], (float)vv[5], (float)vv[6], (float)vv[7]);
                            *(uint2*)kd = k8;
                            *(uint2*)(kd + ps.v_off) = v8;
                        }
                    }
                }
            }
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int d = ch * 8 + i;
                sVt[d * 64 + (((key >> 3) ^ sq_swz(d)) * 8) + (key & 7)] = vv[i];
            }
        }
        __syncthreads();
        float s[4][4];
        float mx = -1e30f;
#pragma unroll
        for (int kt = 0; kt < 4; ++kt) {
            sq_f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            const int krow = kt * 16 + r;
#pragma unroll
            for (int dc = 0; dc < 2; ++dc)
                acc = sq_mfma(*(const f16x8*)(sK + krow * 64 + (((dc * 4 + c) ^ sq_swz(krow)) * 8)), qf[dc], acc);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int key = kb * 64 + kt * 16 + 4 * c + i;
                s[kt][i] = (key <= tq && key < T) ? acc[i] * scale_log2 : -__builtin_inff();
                mx = fmaxf(mx, s[kt][i]);
            }
        }
        mx = fmaxf(mx, __shfl_xor(mx, 16));
        mx = fmaxf(mx, __shfl_xor(mx, 32));
        const float mnew = fmaxf(m, mx);
        const float alpha = __builtin_amdgcn_exp2f(m - mnew);
        l *= alpha;
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) o[dt] *= alpha;
#pragma unroll
        for (int kt = 0; kt < 4; ++kt) {
            sq_f16x4 pv;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float pe = __builtin_amdgcn_exp2f(s[kt][i] - mnew);
                l += pe;
                pv[i] = sq_h(pe);
            }
            *(sq_f16x4*)(Pw + r * 64 + (((kt * 2 + (c >> 1)) ^ sq_swz(r)) * 8) + (c & 1) * 4) = pv;
        }
        m = mnew;
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the wave's own P: every lane's writes have landed
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const f16x8 pf = *(const f16x8*)(Pw + r * 64 + (((ks * 4 + c) ^ sq_swz(r)) * 8));
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) {
                const int drow = dt * 16 + r;
                o[dt] = sq_mfma(*(const f16x8*)(sVt + drow * 64 + (((ks * 4 + c) ^ sq_swz(drow)) * 8)), pf, o[dt]);
            }
        }
    }
    l += __shfl_xor(l, 16);
    l += __shfl_xor(l, 32);
    if (tq >= T) return;
    const float inv = 1.0f / l;
    _Float16* orow = obase + (int64_t)(tq - past) * out_stride;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
        sq_f16x4 v;
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = sq_h(o[dt][i] * inv);
        *(sq_f16x4*)(orow + dt * 16 + 4 * c) = v;
    }
}

__global__ __launch_bounds__(256) void seq_attn_kernel(const _Float16* __restrict__ qkv, int64_t qkv_stride,
                                                       _Float16* __restrict__ out, int64_t out_stride, int T, int H,
                                                       float scale_log2) {
    const int nqb = (T + 63) / 64;
    const int qb = nqb - 1 - (int)(blockIdx.x % nqb);  // the longest query blocks of a pair are dispatched first
    const int bh = (int)(blockIdx.x / nqb);
    const int h = bh % H, b = bh / H;
    seq_attn_block<0>(qkv + (int64_t)b * T * qkv_stride + h * ATT_D, qkv_stride,
                      out + (int64_t)b * T * out_stride + h * ATT_D, out_stride, T, qb, h, H * ATT_D, scale_log2,
                      SeqStore{});
}

// Ragged form: n_seq sequences packed back to back (sequence s = rows seq_start[s] .. seq_start[s + 1] - 1 of the
// R packed rows); workgroup (i, h) serves entry i of the host's block list, (sequence, 64-query block), longest
// blocks first.  A list entry or an offset pair that does not describe a block inside the R rows retires the
// workgroup before it reads a row (uniform, ahead of every barrier).  STORE as in seq_attn_block.
template <int STORE>
__global__ __launch_bounds__(256) void seq_attn_ragged_kernel(const _Float16* __restrict__ qkv, int64_t qkv_stride,
                                                              _Float16* __restrict__ out, int64_t out_stride,
                                                              const int32_t* __restrict__ seq_start, int n_seq, int R,
                                                              const int32_t* __restrict__ blocks, int H,
                                                              float scale_log2, const uint64_t* __restrict__ table,
                                                              int64_t tstride, int max_chunks,
                                                              const int32_t* __restrict__ seq_slot, int n_slots,
                                                              int64_t layer_off) {
    const int i = (int)(blockIdx.x / H), h = (int)(blockIdx.x % H);
    const int s = blocks[2 * i], qb = blocks[2 * i + 1];
    if (s < 0 || s >= n_seq || qb < 0) return;
    const int r0 = seq_start[s], T = seq_start[s + 1] - r0;
    if (r0 < 0 || T < 1 || T > R - r0 || (int64_t)qb * 64 >= T) return;
    SeqStore ps{};
    if constexpr (STORE != 0) {
        const int slot = seq_slot[s];
        if (slot >= 0 && slot < n_slots) {  // (a slot outside the table: attention only, nothing stored)
            ps.table = table + (int64_t)slot * tstride;
            ps.max_chunks = max_chunks;
        }
        ps.layer_off = layer_off;
        ps.v_off = (int64_t)H * 32 * ATT_D;
    }
    seq_attn_block<STORE>(qkv + (int64_t)r0 * qkv_stride + h * ATT_D, qkv_stride,
                          out + (int64_t)r0 * out_stride + h * ATT_D, out_stride, T, qb, h, H * ATT_D, scale_log2, ps);
}

// The ragged form continued from pages (ns_seq_attention_ragged_past, fp16 pages): sequence s has past[s] rows -- a
// multiple of 64 -- in the first past[s] / 32 pages of its table row already, and its packed rows are its absolute
// rows past[s] ..; list entry (s, j) is the 64 new queries from absolute row past[s] + 64 j.  On top of the ragged
// form's guards the workgroup retires, before it reads a row or a page, when past[s] is negative or no multiple of 64,
// when a past page lies at or beyond max_chunks (or the sequence has no table row), or when a past page's entry is
// zero or misaligned: nothing is read through a bad entry.  past[s] == 0 runs the ragged form's instructions.
__global__ __launch_bounds__(256) void seq_attn_ragged_past_kernel(
    const _Float16* __restrict__ qkv, int64_t qkv_stride, _Float16* __restrict__ out, int64_t out_stride,
    const int32_t* __restrict__ seq_start, const int32_t* __restrict__ seq_past, int n_seq, int R,
    const int32_t* __restrict__ blocks, int H, float scale_log2, const uint64_t* __restrict__ table, int64_t tstride,
    int max_chunks, const int32_t* __restrict__ seq_slot, int n_slots, int64_t layer_off) {
    const int i = (int)(blockIdx.x / H), h = (int)(blockIdx.x % H);
    const int s = blocks[2 * i], j = blocks[2 * i + 1];
    if (s < 0 || s >= n_seq || j < 0) return;
    const int r0 = seq_start[s], Tn = seq_start[s + 1] - r0, past = seq_past[s];
    if (r0 < 0 || Tn < 1 || Tn > R - r0 || (int64_t)j * 64 >= Tn) return;
    if (past < 0 || (past & 63) || (past >> 5) > max_chunks || (int64_t)past + Tn > 0x7FFFFFFF) return;
    SeqStore ps{};
    const int slot = seq_slot[s];
    if (slot >= 0 && slot < n_slots) {  // (a slot outside the table: attention only, nothing stored)
        ps.table = table + (int64_t)slot * tstride;
        ps.max_chunks = max_chunks;
    } else if (past > 0) {
        return;
    }
    for (int p = 0; p < (past >> 5); ++p) {
        const uint64_t pg = ps.table[p];
        if (pg == 0 || (pg & 15u)) return;
    }
    ps.layer_off = layer_off;
    ps.v_off = (int64_t)H * 32 * ATT_D;
    ps.past = past;
    seq_attn_block<1, true>(qkv + (int64_t)r0 * qkv_stride + h * ATT_D, qkv_stride,
                            out + (int64_t)r0 * out_stride + h * ATT_D, out_stride, past + Tn, (past >> 6) + j, h,
                            H * ATT_D, scale_log2, ps);
}

}  // namespace nsg

template <class F>
static int decode_attention(const void* d_qkv, int64_t qkv_stride, void* d_k_cache, void* d_v_cache,
                            int64_t cache_b_stride, int64_t cache_h_stride, int64_t cache_chunk_stride,
                            const void* d_k_prefix,
                            const void* d_v_prefix, int64_t prefix_h_stride, int T0, int B, int H, int D, int L0,
                            const int32_t* d_L0, int cap, int window, void* d_out, int64_t out_stride, float scale,
                            void* hip_stream, const uint32_t* d_done = nullptr, int64_t done_stride = 0,
                            const int32_t* d_stop = nullptr) {
    if (d_done && done_stride < 1) return NS_ERR_CONFIG;
    typedef typename F::Elem E;
    if (window < 0) return NS_ERR_CONFIG;
    if (!d_qkv || !d_k_cache || !d_v_cache || !d_out || B <= 0 || H <= 0 || L0 < 0 || T0 < 0) return NS_ERR_CONFIG;
    if (D != nsg::ATT_D) return NS_ERR_UNSUPPORTED;
    constexpr int ALIGN_E = 16 / (int)sizeof(E);  // elements per 16-byte unit of the cache
    if (T0 > 0 && (!d_k_prefix || !d_v_prefix || prefix_h_stride < (int64_t)T0 * D || (prefix_h_stride % ALIGN_E)))
        return NS_ERR_CONFIG;
    if (!d_L0 && L0 < T0) return NS_ERR_CONFIG;
    const uintptr_t align = (uintptr_t)d_qkv | (uintptr_t)d_k_cache | (uintptr_t)d_v_cache | (uintptr_t)d_out |
                            (uintptr_t)(T0 > 0 ? d_k_prefix : d_qkv) | (uintptr_t)(T0 > 0 ? d_v_prefix : d_qkv);
    if (cache_chunk_stride == 0) cache_chunk_stride = 32LL * D;  // plain layout: rows contiguous per (b, h)
    if ((align & 15u) || (qkv_stride & 7) || (out_stride & 7) || (cache_b_stride % ALIGN_E) ||
        (cache_h_stride % ALIGN_E) || (cache_chunk_stride % ALIGN_E))
        return NS_ERR_CONFIG;  // 16-byte rows
    if (qkv_stride < 3LL * H * D || out_stride < (int64_t)H * D) return NS_ERR_CONFIG;
    // the stream cache holds positions [T0, cap): cap - T0 rows per (stream, head), in 32-row chunks
    if (cap <= T0) return NS_ERR_CONFIG;
    const int64_t nchunks = (cap - T0 + 31) / 32;
    if (cache_chunk_stride == 32LL * D && cache_h_stride >= (int64_t)(cap - T0) * D) {
        // plain: a pair's rows contiguous, pairs apart by the h / b strides
        if (cache_b_stride < (int64_t)H * cache_h_stride) return NS_ERR_CONFIG;
    } else {  // chunked: a plane of B*H chunks per 32 positions
        if (cache_h_stride < 32LL * D || cache_b_stride < (int64_t)H * cache_h_stride ||
            cache_chunk_stride < (int64_t)B * cache_b_stride || nchunks < 1)
            return NS_ERR_CONFIG;
    }
    if (!d_L0 && L0 >= cap) return NS_ERR_CONFIG;
    if ((int64_t)B * H > 0x7FFFFFFF) return NS_ERR_UNSUPPORTED;
    const int pairs = B * H;
    const float scale_log2 = scale * 1.4426950408889634f;
    // The row split per pair (att_split) depends on the key count only, so a stream's output -- and the logits the
    // coder sees -- does not depend on how many other streams share the launch (a cover encoded at B = 4096 is
    // decoded alone).  Pairs per workgroup follow the batch: 8 when there are enough pairs to fill the chip.
    const hipStream_t st = (hipStream_t)hip_stream;
    const _Float16* q = (const _Float16*)d_qkv;
    E *k = (E*)d_k_cache, *v = (E*)d_v_cache;
    _Float16* o = (_Float16*)d_out;
    const E* kp = T0 > 0 ? (const E*)d_k_prefix : k;
    const E* vp = T0 > 0 ? (const E*)d_v_prefix : v;
    if (pairs <= NSG_ATT_SMALL_PAIRS)
        hipLaunchKernelGGL((nsg::decode_attn_kernel<F, 1>), dim3(pairs), dim3(512), 0, st, q, qkv_stride, k, v,
                           cache_b_stride, cache_h_stride, cache_chunk_stride, kp, vp, prefix_h_stride, T0, B, H,
                           L0, d_L0, cap, window, d_done, done_stride, d_stop, o, out_stride, scale_log2);
    else
        hipLaunchKernelGGL((nsg::decode_attn_kernel<F, 8>), dim3(NSG_ATT_HEAD_MAJOR ? H * ((B + 7) / 8) : (pairs + 7) / 8),
                           dim3(512), 0, st, q, qkv_stride, k,
                           v, cache_b_stride, cache_h_stride, cache_chunk_stride, kp, vp, prefix_h_stride, T0, B,
                           H, L0, d_L0, cap, window, d_done, done_stride, d_stop, o, out_stride, scale_log2);
    return hipGetLastError() == hipSuccess ? NS_OK : NS_ERR_HIP;
}

extern "C" int ns_decode_attention(const void* d_qkv, int64_t qkv_stride, void* d_k_cache, void* d_v_cache,
                                   int64_t cache_b_stride, int64_t cache_h_stride, int B, int H, int D, int L0,
                                   void* d_out, int64_t out_stride, float scale, void* hip_stream) {
    return decode_attention<nsg::FmtF16>(d_qkv, qkv_stride, d_k_cache, d_v_cache, cache_b_stride, cache_h_stride, 0,
                                         nullptr, nullptr, 0, 0, B, H, D, L0, nullptr, L0 + 1, 0, d_out, out_stride,
                                         scale, hip_stream);
}

extern "C" int ns_decode_attention_dev(const void* d_qkv, int64_t qkv_stride, void* d_k_cache, void* d_v_cache,
                                       int64_t cache_b_stride, int64_t cache_h_stride, int B, int H, int D,
                                       const int32_t* d_L0, int cap, void* d_out, int64_t out_stride, float scale,
                                       void* hip_stream) {
    if (!d_L0 || cap < 1) return NS_ERR_CONFIG;
    return decode_attention<nsg::FmtF16>(d_qkv, qkv_stride, d_k_cache, d_v_cache, cache_b_stride, cache_h_stride, 0,
                                         nullptr, nullptr, 0, 0, B, H, D, 0, d_L0, cap, 0, d_out, out_stride, scale,
                                         hip_stream);
}

extern "C" int ns_decode_attention_prefix(const void* d_qkv, int64_t qkv_stride, void* d_k_cache, void* d_v_cache,
                                          int64_t cache_b_stride, int64_t cache_h_stride, int64_t cache_chunk_stride,
                                          const void* d_k_prefix, const void* d_v_prefix, int64_t prefix_h_stride,
                                          int T0, int B, int H, int D, int L0, const int32_t* d_L0, int cap, int window,
                                          void* d_out, int64_t out_stride, float scale, void* hip_stream) {
    return decode_attention<nsg::FmtF16>(d_qkv, qkv_stride, d_k_cache, d_v_cache, cache_b_stride, cache_h_stride,
                                         cache_chunk_stride, d_k_prefix, d_v_prefix, prefix_h_stride, T0, B, H, D,
                                         d_L0 ? 0 : L0, d_L0, cap, window, d_out, out_stride, scale, hip_stream);
}

extern "C" int ns_decode_attention_fp8(const void* d_qkv, int64_t qkv_stride, void* d_k_cache, void* d_v_cache,
                                       int64_t cache_b_stride, int64_t cache_h_stride, int64_t cache_chunk_stride,
                                       const void* d_k_prefix, const void* d_v_prefix, int64_t prefix_h_stride,
                                       int T0, int B, int H, int D, int L0, const int32_t* d_L0, int cap, int window,
                                       void* d_out, int64_t out_stride, float scale, void* hip_stream) {
    return decode_attention<nsg::FmtF8>(d_qkv, qkv_stride, d_k_cache, d_v_cache, cache_b_stride, cache_h_stride,
                                        cache_chunk_stride, d_k_prefix, d_v_prefix, prefix_h_stride, T0, B, H, D,
                                        d_L0 ? 0 : L0, d_L0, cap, window, d_out, out_stride, scale, hip_stream);
}

extern "C" int ns_decode_attention_ex(const void* d_qkv, int64_t qkv_stride, void* d_k_cache, void* d_v_cache,
                                      int64_t cache_b_stride, int64_t cache_h_stride, int64_t cache_chunk_stride,
                                      const void* d_k_prefix, const void* d_v_prefix, int64_t prefix_h_stride, int T0,
                                      int B, int H, int D, int L0, const int32_t* d_L0, int cap, int window,
                                      int kv_format, const uint32_t* d_done, int64_t done_stride,
                                      const int32_t* d_stop, void* d_out, int64_t out_stride, float scale,
                                      void* hip_stream) {
    if (kv_format == NS_KV_FP16)
        return decode_attention<nsg::FmtF16>(d_qkv, qkv_stride, d_k_cache, d_v_cache, cache_b_stride, cache_h_stride,
                                             cache_chunk_stride, d_k_prefix, d_v_prefix, prefix_h_stride, T0, B, H, D,
                                             d_L0 ? 0 : L0, d_L0, cap, window, d_out, out_stride, scale, hip_stream,
                                             d_done, done_stride, d_stop);
    if (kv_format == NS_KV_FP8)
        return decode_attention<nsg::FmtF8>(d_qkv, qkv_stride, d_k_cache, d_v_cache, cache_b_stride, cache_h_stride,
                                            cache_chunk_stride, d_k_prefix, d_v_prefix, prefix_h_stride, T0, B, H, D,
                                            d_L0 ? 0 : L0, d_L0, cap, window, d_out, out_stride, scale, hip_stream,
                                            d_done, done_stride, d_stop);
    return NS_ERR_CONFIG;
}

template <class F>
static int paged_attention(nsg::PagedArgs a, void* hip_stream) {
    const hipStream_t st = (hipStream_t)hip_stream;
    const int pairs = a.B * a.H;
    if (pairs <= NSG_ATT_SMALL_PAIRS)
        hipLaunchKernelGGL((nsg::paged_attn_kernel<F, 1>), dim3(pairs), dim3(512), 0, st, a);
    else
        hipLaunchKernelGGL((nsg::paged_attn_kernel<F, 8>), dim3(a.H * ((a.B + 7) / 8)), dim3(512), 0, st, a);
    return hipGetLastError() == hipSuccess ? NS_OK : NS_ERR_HIP;
}

extern "C" int ns_decode_attention_paged(const void* d_qkv, int64_t qkv_stride, const uint64_t* d_page_table,
                                         int64_t table_stride, int max_chunks, int64_t layer_offset,
                                         const void* d_k_prefix,
                                         const void* d_v_prefix, int64_t prefix_h_stride, int T0, int B, int H, int D,
                                         const int32_t* d_lens, int window, int kv_format, const uint32_t* d_done,
                                         int64_t done_stride, const int32_t* d_stop, void* d_out, int64_t out_stride,
                                         float scale, void* hip_stream) {
    if (!d_qkv || !d_page_table || !d_lens || !d_out || B <= 0 || H <= 0 || T0 < 0 || layer_offset < 0 || window < 0)
        return NS_ERR_CONFIG;
    if (D != nsg::ATT_D) return NS_ERR_UNSUPPORTED;
    if (kv_format != NS_KV_FP16 && kv_format != NS_KV_FP8) return NS_ERR_CONFIG;
    if (max_chunks < 1 || table_stride < max_chunks || (d_done && done_stride < 1)) return NS_ERR_CONFIG;
    const int64_t esz = kv_format == NS_KV_FP8 ? 1 : 2;
    if (T0 > 0 && (!d_k_prefix || !d_v_prefix || prefix_h_stride < (int64_t)T0 * D || ((prefix_h_stride * esz) & 15)))
        return NS_ERR_CONFIG;
    const uintptr_t align = (uintptr_t)d_qkv | (uintptr_t)d_out | (uintptr_t)(T0 > 0 ? d_k_prefix : d_qkv) |
                            (uintptr_t)(T0 > 0 ? d_v_prefix : d_qkv);
    if ((align & 15u) || (qkv_stride & 7) || (out_stride & 7) || ((uintptr_t)d_lens & 3u) ||
        ((uintptr_t)d_page_table & 7u))  // table entries are read one uint64 at a time: any row of a table works
        return NS_ERR_CONFIG;
    if (qkv_stride < 3LL * H * D || out_stride < (int64_t)H * D) return NS_ERR_CONFIG;
    if ((int64_t)B * H > 0x7FFFFFFF) return NS_ERR_UNSUPPORTED;
    nsg::PagedArgs a;
    a.qkv = (const _Float16*)d_qkv;
    a.qkv_stride = qkv_stride;
    a.table = d_page_table;
    a.tstride = table_stride;
    a.max_chunks = max_chunks;
    a.v_off = (int64_t)H * 32 * D;
    if (layer_offset % (16 / esz)) return NS_ERR_CONFIG;  // 16-byte rows
    a.layer_off = layer_offset;
    a.kp = T0 > 0 ? d_k_prefix : d_qkv;
    a.vp = T0 > 0 ? d_v_prefix : d_qkv;
    a.ph = prefix_h_stride;
    a.T0 = T0;
    a.B = B;
    a.H = H;
    a.lens = d_lens;
    a.window = window;
    a.done = d_done;
    a.done_stride = done_stride;
    a.stop = d_stop;
    a.out = (_Float16*)d_out;
    a.out_stride = out_stride;
    a.scale_log2 = scale * 1.4426950408889634f;
    return kv_format == NS_KV_FP8 ? paged_attention<nsg::FmtF8>(a, hip_stream)
                                  : paged_attention<nsg::FmtF16>(a, hip_stream);
}

template <class F, int CTMAX>
static int paged_attention_chunk(const nsg::PagedArgs& a, int C, const int32_t* d_count, void* hip_stream) {
    const hipStream_t st = (hipStream_t)hip_stream;
    const dim3 grid(a.B * a.H);
    // CT = queries a wave keeps in registers at once (the smallest power of two >= C, at most CTMAX: more queries
    // stream their chunks again); placement only, a query's arithmetic does not depend on it
    if (C <= 1)
        hipLaunchKernelGGL((nsg::paged_attn_chunk_kernel<F, 1, 8>), grid, dim3(512), 0, st, a, C, d_count);
    else if (C <= 2)
        hipLaunchKernelGGL((nsg::paged_attn_chunk_kernel<F, 2, 8>), grid, dim3(512), 0, st, a, C, d_count);
    else if (C <= 4)
        hipLaunchKernelGGL((nsg::paged_attn_chunk_kernel<F, 4, 8>), grid, dim3(512), 0, st, a, C, d_count);
    else if (C <= 8 || CTMAX <= 8)
        hipLaunchKernelGGL((nsg::paged_attn_chunk_kernel<F, 8, 8>), grid, dim3(512), 0, st, a, C, d_count);
    else
        hipLaunchKernelGGL((nsg::paged_attn_chunk_kernel<F, CTMAX, 4>), grid, dim3(256), 0, st, a, C, d_count);
    return hipGetLastError() == hipSuccess ? NS_OK : NS_ERR_HIP;
}

extern "C" int ns_decode_attention_paged_chunk(const void* d_qkv, int64_t qkv_stride, const uint64_t* d_page_table,
                                               int64_t table_stride, int max_chunks, int64_t layer_offset,
                                               const void* d_k_prefix, const void* d_v_prefix,
                                               int64_t prefix_h_stride, int T0, int B, int H, int D,
                                               const int32_t* d_lens, int window, int kv_format, int C,
                                               const int32_t* d_count, void* d_out, int64_t out_stride, float scale,
                                               void* hip_stream) {
    if (!d_qkv || !d_page_table || !d_lens || !d_count || !d_out || B <= 0 || H <= 0 || T0 < 0 || layer_offset < 0 ||
        window < 0)
        return NS_ERR_CONFIG;
    if (C < 1 || C > nsg::ATT_CHUNK_MAX || D != nsg::ATT_D) return NS_ERR_CONFIG;
    if (window > 0) return NS_ERR_UNSUPPORTED;
    if (kv_format != NS_KV_FP16 && kv_format != NS_KV_FP8) return NS_ERR_CONFIG;
    if (max_chunks < 1 || table_stride < max_chunks) return NS_ERR_CONFIG;
    const int64_t esz = kv_format == NS_KV_FP8 ? 1 : 2;
    if (T0 > 0 && (!d_k_prefix || !d_v_prefix || prefix_h_stride < (int64_t)T0 * D || ((prefix_h_stride * esz) & 15)))
        return NS_ERR_CONFIG;
    const uintptr_t align = (uintptr_t)d_qkv | (uintptr_t)d_out | (uintptr_t)(T0 > 0 ? d_k_prefix : d_qkv) |
                            (uintptr_t)(T0 > 0 ? d_v_prefix : d_qkv);
    if ((align & 15u) || (qkv_stride & 7) || (out_stride & 7) || (((uintptr_t)d_lens | (uintptr_t)d_count) & 3u) ||
        ((uintptr_t)d_page_table & 7u))
        return NS_ERR_CONFIG;
    if (qkv_stride < 3LL * H * D || out_stride < (int64_t)H * D) return NS_ERR_CONFIG;
    if ((int64_t)B * H > 0x7FFFFFFF) return NS_ERR_UNSUPPORTED;
    if (layer_offset % (16 / esz)) return NS_ERR_CONFIG;  // 16-byte rows
    nsg::PagedArgs a;
    a.qkv = (const _Float16*)d_qkv;
    a.qkv_stride = qkv_stride;
    a.table = d_page_table;
    a.tstride = table_stride;
    a.max_chunks = max_chunks;
    a.v_off = (int64_t)H * 32 * D;
    a.layer_off = layer_offset;
    a.kp = T0 > 0 ? d_k_prefix : d_qkv;
    a.vp = T0 > 0 ? d_v_prefix : d_qkv;
    a.ph = prefix_h_stride;
    a.T0 = T0;
    a.B = B;
    a.H = H;
    a.lens = d_lens;
    a.window = 0;
    a.done = nullptr;
    a.done_stride = 0;
    a.stop = nullptr;
    a.out = (_Float16*)d_out;
    a.out_stride = out_stride;
    a.scale_log2 = scale * 1.4426950408889634f;
    return kv_format == NS_KV_FP8 ? paged_attention_chunk<nsg::FmtF8, 8>(a, C, d_count, hip_stream)
                                  : paged_attention_chunk<nsg::FmtF16, 16>(a, C, d_count, hip_stream);
}

extern "C" int ns_quantize_fp8(const void* d_src, void* d_dst, int64_t n, void* hip_stream) {
    if (!d_src || !d_dst || n < 0 || (n & 3) || (((uintptr_t)d_src | (uintptr_t)d_dst) & 7u)) return NS_ERR_CONFIG;
    if (n == 0) return NS_OK;
    const int64_t n4 = n / 4;
    hipLaunchKernelGGL(nsg::quantize_fp8_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0,
                       (hipStream_t)hip_stream, (const _Float16*)d_src, (uint32_t*)d_dst, n4);
    return hipGetLastError() == hipSuccess ? NS_OK : NS_ERR_HIP;
}

extern "C" int ns_seq_attention(const void* d_qkv, int64_t qkv_stride, void* d_out, int64_t out_stride, int B, int T,
                                int H, int D, float scale, void* hip_stream) {
    if (!d_qkv || !d_out || B < 1 || T < 1 || H < 1) return NS_ERR_CONFIG;
    if (D != nsg::ATT_D) return NS_ERR_UNSUPPORTED;
    if (qkv_stride < 3LL * H * D || out_stride < (int64_t)H * D || (qkv_stride & 7) || (out_stride & 3) ||
        (((uintptr_t)d_qkv | (uintptr_t)d_out) & 15u))
        return NS_ERR_CONFIG;
    const int64_t nwg = (int64_t)B * H * ((T + 63) / 64);
    if (nwg > 0x7FFFFFFF) return NS_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(nsg::seq_attn_kernel, dim3((unsigned)nwg), dim3(256), 0, (hipStream_t)hip_stream,
                       (const _Float16*)d_qkv, qkv_stride, (_Float16*)d_out, out_stride, T, H,
                       scale * 1.4426950408889634f);
    return hipGetLastError() == hipSuccess ? NS_OK : NS_ERR_HIP;
}

extern "C" int ns_seq_attention_ragged(const void* d_qkv, int64_t qkv_stride, void* d_out, int64_t out_stride,
                                       const int32_t* d_seq_start, int n_seq, int R, const int32_t* d_blocks,
                                       int nblk, int H, int D, float scale, const uint64_t* d_page_table,
                                       int64_t table_stride, int max_chunks, const int32_t* d_seq_slot, int n_slots,
                                       int64_t layer_offset, int kv_format, void* hip_stream) {
    if (!d_qkv || !d_out || !d_seq_start || !d_blocks || n_seq < 1 || R < n_seq || nblk < 1 || H < 1)
        return NS_ERR_CONFIG;
    if (D != nsg::ATT_D) return NS_ERR_UNSUPPORTED;
    if (qkv_stride < 3LL * H * D || out_stride < (int64_t)H * D || (qkv_stride & 7) || (out_stride & 3) ||
        (((uintptr_t)d_qkv | (uintptr_t)d_out) & 15u) || (((uintptr_t)d_seq_start | (uintptr_t)d_blocks) & 3u))
        return NS_ERR_CONFIG;
    if (nblk > (R + 63) / 64 + n_seq) return NS_ERR_CONFIG;  // more entries than the R rows can have blocks
    if ((int64_t)nblk * H > 0x7FFFFFFF) return NS_ERR_UNSUPPORTED;
    const dim3 grid((unsigned)((int64_t)nblk * H)), wg(256);
    const hipStream_t st = (hipStream_t)hip_stream;
    const _Float16* q = (const _Float16*)d_qkv;
    _Float16* o = (_Float16*)d_out;
    const float sl2 = scale * 1.4426950408889634f;
    if (!d_page_table) {
        hipLaunchKernelGGL(nsg::seq_attn_ragged_kernel<0>, grid, wg, 0, st, q, qkv_stride, o, out_stride, d_seq_start,
                           n_seq, R, d_blocks, H, sl2, nullptr, 0, 0, nullptr, 0, 0);
        return hipGetLastError() == hipSuccess ? NS_OK : NS_ERR_HIP;
    }
    if (kv_format != NS_KV_FP16 && kv_format != NS_KV_FP8) return NS_ERR_CONFIG;
    if (!d_seq_slot || n_slots < 1 || max_chunks < 1 || table_stride < max_chunks || layer_offset < 0 ||
        ((uintptr_t)d_page_table & 7u) || ((uintptr_t)d_seq_slot & 3u))
        return NS_ERR_CONFIG;
    if (layer_offset % (kv_format == NS_KV_FP8 ? 16 : 8)) return NS_ERR_CONFIG;  // 16-byte rows
    if (kv_format == NS_KV_FP8)
        hipLaunchKernelGGL(nsg::seq_attn_ragged_kernel<2>, grid, wg, 0, st, q, qkv_stride, o, out_stride, d_seq_start,
                           n_seq, R, d_blocks, H, sl2, d_page_table, table_stride, max_chunks, d_seq_slot, n_slots,
                           layer_offset);
    else
        hipLaunchKernelGGL(nsg::seq_attn_ragged_kernel<1>, grid, wg, 0, st, q, qkv_stride, o, out_stride, d_seq_start,
                           n_seq, R, d_blocks, H, sl2, d_page_table, table_stride, max_chunks, d_seq_slot, n_slots,
                           layer_offset);
    return hipGetLastError() == hipSuccess ? NS_OK : NS_ERR_HIP;
}

extern "C" int ns_seq_attention_ragged_past(const void* d_qkv, int64_t qkv_stride, void* d_out, int64_t out_stride,
                                            const int32_t* d_seq_start, const int32_t* d_seq_past, int n_seq, int R,
                                            const int32_t* d_blocks, int nblk, int H, int D, float scale,
                                            const uint64_t* d_page_table, int64_t table_stride, int max_chunks,
                                            const int32_t* d_seq_slot, int n_slots, int64_t layer_offset,
                                            int kv_format, void* hip_stream) {
    if (!d_qkv || !d_out || !d_seq_start || !d_blocks || n_seq < 1 || R < n_seq || nblk < 1 || H < 1)
        return NS_ERR_CONFIG;
    if (D != nsg::ATT_D || !d_page_table || !d_seq_past) return NS_ERR_CONFIG;
    if (kv_format == NS_KV_FP8) return NS_ERR_UNSUPPORTED;  // fp8 pages are no bit copies of the qkv rows
    if (kv_format != NS_KV_FP16) return NS_ERR_CONFIG;
    if (qkv_stride < 3LL * H * D || out_stride < (int64_t)H * D || (qkv_stride & 7) || (out_stride & 3) ||
        (((uintptr_t)d_qkv | (uintptr_t)d_out) & 15u) ||
        (((uintptr_t)d_seq_start | (uintptr_t)d_blocks | (uintptr_t)d_seq_past) & 3u))
        return NS_ERR_CONFIG;
    if (nblk > (R + 63) / 64 + n_seq) return NS_ERR_CONFIG;  // more entries than the R rows can have blocks
    if ((int64_t)nblk * H > 0x7FFFFFFF) return NS_ERR_UNSUPPORTED;
    if (!d_seq_slot || n_slots < 1 || max_chunks < 1 || table_stride < max_chunks || layer_offset < 0 ||
        ((uintptr_t)d_page_table & 7u) || ((uintptr_t)d_seq_slot & 3u) || (layer_offset % 8))
        return NS_ERR_CONFIG;
    hipLaunchKernelGGL(nsg::seq_attn_ragged_past_kernel, dim3((unsigned)((int64_t)nblk * H)), dim3(256), 0,
                       (hipStream_t)hip_stream, (const _Float16*)d_qkv, qkv_stride, (_Float16*)d_out, out_stride,
                       d_seq_start, d_seq_past, n_seq, R, d_blocks, H, scale * 1.4426950408889634f, d_page_table,
                       table_stride, max_chunks, d_seq_slot, n_slots, layer_offset);
    return hipGetLastError() == hipSuccess ? NS_OK : NS_ERR_HIP;
}

// ---------------------------------------------------------------------------------------------------------------
// ns_kv_copy_rows: the head rows of one KV page into another, every layer (a context's KV pages shared among the
// messages that carry it, lm/kvpages.py: the context's last, partly filled page is copied into each holder's own
// first page, which the holder then appends into).  One workgroup per (pair, layer): the layer's block is 2H pieces
// ([K|V][H]) of 32 rows; the first `rows` rows of a piece are rows * row_vecs contiguous 16-byte vectors (a row is
// 128 B in fp16, 64 B in fp8), so consecutive lanes move consecutive vectors.  Bytes are moved as they are.
namespace nsg {
__global__ __launch_bounds__(256) void kv_copy_rows_kernel(const uint64_t* __restrict__ src,
                                                           const uint64_t* __restrict__ dst,
                                                           const int32_t* __restrict__ rows, int n, int n_layer,
                                                           int64_t layer_bytes, int pieces, int row_vecs) {
    const int pair = (int)(blockIdx.x / (unsigned)n_layer), layer = (int)(blockIdx.x % (unsigned)n_layer);
    if (pair >= n) return;
    const uint64_t s = src[pair], d = dst[pair];
    const int r = rows[pair];
    if (!s || !d || ((s | d) & 15u) || s == d || r <= 0 || r > 32) return;
    const uint4* sp = (const uint4*)(s + (uint64_t)layer * (uint64_t)layer_bytes);
    uint4* dp = (uint4*)(d + (uint64_t)layer * (uint64_t)layer_bytes);
    const int nv = r * row_vecs, piece_vecs = 32 * row_vecs;  // nv <= 256
    for (int i = (int)threadIdx.x; i < pieces * nv; i += 256) {
        const int p = i / nv, v = i - p * nv;
        dp[p * piece_vecs + v] = sp[p * piece_vecs + v];
    }
}
}  // namespace nsg

extern "C" int ns_kv_copy_rows(const uint64_t* d_src, const uint64_t* d_dst, const int32_t* d_rows, int n,
                               int n_layer, int64_t layer_stride, int H, int D, int kv_format, void* hip_stream) {
    if (n < 0 || n_layer < 1 || H < 1 || H > 4096 || D < 1) return NS_ERR_CONFIG;
    if (D != nsg::ATT_D) return NS_ERR_UNSUPPORTED;
    if (kv_format != NS_KV_FP16 && kv_format != NS_KV_FP8) return NS_ERR_CONFIG;
    const int esize = kv_format == NS_KV_FP8 ? 1 : 2;
    if (layer_stride < 0 || layer_stride % (16 / esize)) return NS_ERR_CONFIG;  // 16-byte vectors
    if (n_layer > 1 && layer_stride < 2LL * H * 32 * D) return NS_ERR_CONFIG;  // layers' blocks would overlap
    if (n == 0) return NS_OK;
    if (!d_src || !d_dst || !d_rows || (((uintptr_t)d_src | (uintptr_t)d_dst) & 7u) || ((uintptr_t)d_rows & 3u))
        return NS_ERR_CONFIG;
    if ((int64_t)n * n_layer > 0x7FFFFFFF) return NS_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(nsg::kv_copy_rows_kernel, dim3((unsigned)((int64_t)n * n_layer)), dim3(256), 0,
                       (hipStream_t)hip_stream, d_src, d_dst, d_rows, n, n_layer, layer_stride * esize, 2 * H,
                       D * esize / 16);
    return hipGetLastError() == hipSuccess ? NS_OK : NS_ERR_HIP;
}
