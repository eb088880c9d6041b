// Per-row log-softmax scores (include/nsg_score.h): nll of the label and the entropy of the row, for the
// cover-text quality guard's perplexity / average-entropy metrics.
//
// One wavefront per row; lane l reads 16-byte vectors l, l+64, ... of the row (coalesced 1 KiB wave loads,
// non-temporal: every row is read exactly once).  Per lane an online softmax over vectors: the vector max
// rescales the running sums once per vector, so the loop costs one extra exp per 4 (fp32) / 8 (fp16) elements.
// The 64 lane states are merged in float64.

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "nsg_coder.h"
#include "nsg_score.h"

namespace nsg {

constexpr int SC_WAVES = 4;  // rows per 256-thread workgroup

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

template <typename T>
struct ScoreVec;

template <>
struct ScoreVec<float> {
    static constexpr int N = 4;
    typedef f32x4 V;
    __device__ static void load(const char* p, float* x) {
        const V v = __builtin_nontemporal_load((const V*)p);
        x[0] = v.x;
        x[1] = v.y;
        x[2] = v.z;
        x[3] = v.w;
    }
    __device__ static float at(const char* row, int j) { return ((const float*)row)[j]; }
};

template <>
struct ScoreVec<_Float16> {
    static constexpr int N = 8;
    typedef f16x8 V;
    __device__ static void load(const char* p, float* x) {
        const V v = __builtin_nontemporal_load((const V*)p);
#pragma unroll
        for (int i = 0; i < 8; ++i) x[i] = (float)v[i];
    }
    __device__ static float at(const char* row, int j) { return (float)((const _Float16*)row)[j]; }
};

template <typename T>
__global__ __launch_bounds__(64 * SC_WAVES) void score_rows_kernel(const char* __restrict__ logits, int64_t ld,
                                                                  int64_t nrows, int V,
                                                                  const int32_t* __restrict__ labels,
                                                                  double* __restrict__ nll, double* __restrict__ ent) {
    constexpr int N = ScoreVec<T>::N;
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * SC_WAVES + (threadIdx.x >> 6);
    if (r >= nrows) return;
    const char* row = logits + r * ld * (int64_t)sizeof(T);
    const int nvec = V / N;  // full vectors; the tail (V % N ids) is handled element-wise below
    // lane state: m = running max, s = sum e^(x - m), u = sum e^(x - m) (x - m)
    float m = -INFINITY, s = 0.0f, u = 0.0f;
    auto rebase = [&](float mv) {  // new max mv > m: u' = a (u + s (m - mv)), s' = a s, a = e^(m - mv)
        if (s > 0.0f) {
            const float a = __expf(m - mv);
            u = a * fmaf(s, m - mv, u);
            s *= a;
        }
        m = mv;
    };
    for (int v = lane; v < nvec; v += 64) {
        float x[N];
        ScoreVec<T>::load(row + (int64_t)v * N * sizeof(T), x);
        float mv = x[0];
#pragma unroll
        for (int i = 1; i < N; ++i) mv = fmaxf(mv, x[i]);
        if (mv > m) rebase(mv);
#pragma unroll
        for (int i = 0; i < N; ++i) {
            const float d = x[i] - m;
            const float e = __expf(d);
            s += e;
            u = fmaf(e, d, u);
        }
    }
    for (int j = nvec * N + lane; j < V; j += 64) {  // ragged tail (V % N ids)
        const float x = ScoreVec<T>::at(row, j);
        if (x > m) rebase(x);
        const float d = x - m;
        const float e = __expf(d);
        s += e;
        u = fmaf(e, d, u);
    }
    double M = (double)m, S = (double)s, U = (double)u;
    for (int off = 32; off >= 1; off >>= 1) {
        const double Mo = __shfl_xor(M, off), So = __shfl_xor(S, off), Uo = __shfl_xor(U, off);
        const double Mn = fmax(M, Mo);
        const double fa = (S > 0.0) ? exp(M - Mn) : 0.0, fo = (So > 0.0) ? exp(Mo - Mn) : 0.0;
        // u relative to Mn: sum e_i (x_i - Mn) = f*(u + s*(M - Mn))
        U = (S > 0.0 ? fa * (U + S * (M - Mn)) : 0.0) + (So > 0.0 ? fo * (Uo + So * (Mo - Mn)) : 0.0);
        S = fa * S + fo * So;
        M = Mn;
    }
    if (lane == 0) {
        const double lse = M + log(S);
        // entropy = lse - sum p x = -(sum e (x - M))/S + log S
        if (ent) ent[r] = log(S) - U / S;
        if (nll) {
            const int lab = labels ? labels[r] : -1;
            nll[r] = (lab >= 0 && lab < V) ? lse - (double)ScoreVec<T>::at(row, lab) : 0.0;
        }
    }
}

// ------------------------------------------------------------------------------------------- fused head + score
// ns_lm_head_score: the vocabulary-wide head GEMM with the row scores as its epilogue -- no [M, V] logits array.
//
// A workgroup of 4 waves (2 x 2, 64 x 64 each) owns 128 activation rows and walks a SPAN of HS_SPAN_TILES
// consecutive 128-column tiles.  Every 16 x 16 accumulator fragment is the canonical one-chain MFMA sum of
// nsg_lm.hip (v_mfma_f32_16x16x32_f16, weight row in MFMA row position, K tiles of 64 in order from zero, the two
// 32-wide k-steps of a tile in order): the bits ns_lm_gemm stores with NS_LM_EPI_STORE_F32, staged exactly as its
// two-buffer 128 x 128 tiles are (global_load_lds, rows XOR-swizzled in 16-byte chunks).  K with more than one
// chain (K > 1024) is refused by the host.
//
// Instead of storing a tile, a lane folds the 4 consecutive columns it holds of each of its 4 rows into the row's
// online-softmax state (m, s, u) of score_rows_kernel, fragment after fragment, tile after tile; after the span
// the 4 lanes of a row are merged (xor 16, xor 32), then the two waves that share the rows through LDS, and one
// (m, s, u) per (row, span) goes to the work buffer.  The lane that holds column label[row] keeps that logit and
// writes it after the span: one write per row in the whole grid.  head_merge_kernel then merges a row's spans in
// ascending order in float64.
//
// Batch invariance: the span cut (HS_SPAN_TILES tiles of 128 columns, from column 0), the column a lane holds and
// every merge order are functions of V only; rows never meet.  A row's outputs have the same bits at M = 1 and in
// any batch.
namespace hs {

typedef _Float16 f16;

constexpr int BN = 128, BM = 128, BK = 64;
constexpr int ROWS = BN + BM;       // staged rows per K-tile (weights first, then activations)
constexpr int NT = 256;             // 4 waves
constexpr int GL = ROWS * 8 / NT;   // 16-byte DMA instructions per thread per K-tile
constexpr int HS_SPAN_TILES = 4;    // column tiles per span (by nothing but this constant)
constexpr int HS_MAX_K = 1024;      // one accumulator chain (k_chains(K) == 1 in nsg_lm.hip)

__device__ __forceinline__ f32x4 mfma16(f16x8 a, f16x8 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
}

// fp32 -> fp16 with the fp32 value pinned first (as in nsg_lm.hip: no fused conversion of the producing op)
__device__ __forceinline__ f16 to_f16(float v) {
    asm volatile("" : "+v"(v));
    return (f16)v;
}

__device__ __forceinline__ int swz(int row) { return (row >> 1) & 7; }

template <int N_>
__device__ __forceinline__ void wait_vm() {
    static_assert(N_ >= 0 && N_ < 64, "vmcnt range");
    __builtin_amdgcn_s_waitcnt((N_ & 15) | (7 << 4) | (15 << 8) | ((N_ >> 4) << 14));
}

__device__ __forceinline__ void lds_fence_barrier() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}

// (m, s, u) <- merge of (m, s, u) and (mo, so, uo): the lane merge of score_rows_kernel (an empty side has s = 0)
template <typename F>
__device__ __forceinline__ void merge_state(F& m, F& s, F& u, F mo, F so, F uo) {
    const F mn = m > mo ? m : mo;
    F fa, fo;
    if constexpr (sizeof(F) == 8) {
        fa = s > 0 ? exp(m - mn) : 0;
        fo = so > 0 ? exp(mo - mn) : 0;
    } else {
        fa = s > 0 ? __expf(m - mn) : 0;
        fo = so > 0 ? __expf(mo - mn) : 0;
    }
    u = (s > 0 ? fa * (u + s * (m - mn)) : 0) + (so > 0 ? fo * (uo + so * (mo - mn)) : 0);
    s = fa * s + fo * so;
    m = mn;
}

template <bool F16OUT>
__global__ __launch_bounds__(NT) void head_score_kernel(const f16* __restrict__ X, int64_t ldx,
                                                        const f16* __restrict__ Wt, int64_t ldw, int M, int V, int K,
                                                        const int32_t* __restrict__ labels, f32x4* __restrict__ part,
                                                        float* __restrict__ xlab) {
    constexpr int FN = 4, FM = 4;  // 16 x 16 fragments per wave: 64 columns x 64 rows
    __shared__ __attribute__((aligned(16))) char smem[2 * ROWS * 128];
    __shared__ float s_red[2][64][3];

    const int span = blockIdx.y;
    const int m0 = blockIdx.x * BM;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wn = wave >> 1, wm = wave & 1;
    const int fr = lane & 15, fc = lane >> 4;
    const int tiles_n = (V + BN - 1) / BN;
    const int t_begin = span * HS_SPAN_TILES, t_end = min(t_begin + HS_SPAN_TILES, tiles_n);
    const int KT = K / BK;

    // the label of each of the lane's 4 rows (-1: none, or outside [0, V))
    int lab[FM];
#pragma unroll
    for (int j = 0; j < FM; ++j) {
        const int row = m0 + wm * 64 + j * 16 + fr;
        int l = (labels && row < M) ? labels[row] : -1;
        lab[j] = (l >= 0 && l < V) ? l : -1;
    }
    float rm[FM], rs[FM], ru[FM], xl[FM];
    bool have[FM];
#pragma unroll
    for (int j = 0; j < FM; ++j) {
        rm[j] = -INFINITY;
        rs[j] = 0.0f;
        ru[j] = 0.0f;
        xl[j] = 0.0f;
        have[j] = false;
    }

    // staging: instruction g of wave w fills LDS rows q*8 .. q*8+7, q = g*4 + w; lane -> row q*8 + lane/8, physical
    // chunk lane%8 = logical chunk (lane%8) ^ swz(row).  Rows past V / M read the last valid row (never past the
    // operands); their results are dropped below.
    const f16* src[GL];
    int lds_off[GL];
#pragma unroll
    for (int g = 0; g < GL; ++g) lds_off[g] = (g * 4 + wave) * 8 * 128;

    for (int t = t_begin; t < t_end; ++t) {  // uniform bounds: every wave walks the same tiles
        const int n0 = t * BN;
#pragma unroll
        for (int g = 0; g < GL; ++g) {
            const int row = (g * 4 + wave) * 8 + (lane >> 3);
            const int chunk = (lane & 7) ^ swz(row);
            if (row < BN)
                src[g] = Wt + (int64_t)min(n0 + row, V - 1) * ldw + chunk * 8;
            else
                src[g] = X + (int64_t)min(m0 + row - BN, M - 1) * ldx + chunk * 8;
        }
        auto stage = [&](int kt, int buf) {
#pragma unroll
            for (int g = 0; g < GL; ++g)
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src[g] + kt * BK),
                                                 (__attribute__((address_space(3))) void*)(smem + buf * ROWS * 128 +
                                                                                           lds_off[g]),
                                                 16, 0, 0);
        };
        f32x4 acc[FN][FM];
#pragma unroll
        for (int i = 0; i < FN; ++i)
#pragma unroll
            for (int j = 0; j < FM; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
        stage(0, 0);
        int buf = 0;
        for (int kt = 0; kt < KT; ++kt) {
            // two buffers: issue tile kt+1, then wait until this thread's copies of tile kt landed
            if (kt + 1 < KT) {
                stage(kt + 1, buf ^ 1);
                wait_vm<GL>();
            } else {
                wait_vm<0>();
            }
            __builtin_amdgcn_s_barrier();  // ... and every other wave's
            asm volatile("" ::: "memory");
            const char* base = smem + buf * ROWS * 128;
            f16x8 a[2][FN], b[2][FM];
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) {
                const int ch = kk * 4 + fc;
#pragma unroll
                for (int i = 0; i < FN; ++i) {
                    const int row = wn * 64 + i * 16 + fr;
                    a[kk][i] = *(const f16x8*)(base + row * 128 + ((ch ^ swz(row)) << 4));
                }
#pragma unroll
                for (int j = 0; j < FM; ++j) {
                    const int row = BN + wm * 64 + j * 16 + fr;
                    b[kk][j] = *(const f16x8*)(base + row * 128 + ((ch ^ swz(row)) << 4));
                }
            }
#pragma unroll
            for (int kk = 0; kk < 2; ++kk)
#pragma unroll
                for (int i = 0; i < FN; ++i)
#pragma unroll
                    for (int j = 0; j < FM; ++j) acc[i][j] = mfma16(a[kk][i], b[kk][j], acc[i][j]);
            lds_fence_barrier();  // every wave is done reading this buffer before it is refilled
            buf ^= 1;
        }
        // epilogue: fragment (i, j) holds columns n .. n+3 of row j of the lane; columns >= V contribute nothing
#pragma unroll
        for (int i = 0; i < FN; ++i) {
            const int n = n0 + wn * 64 + i * 16 + 4 * fc;
            if (n >= V) continue;
#pragma unroll
            for (int j = 0; j < FM; ++j) {
                float x[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) x[r] = F16OUT ? (float)to_f16(acc[i][j][r]) : acc[i][j][r];
                float mv = x[0];
#pragma unroll
                for (int r = 1; r < 4; ++r)
                    if (n + r < V) mv = fmaxf(mv, x[r]);
                if (mv > rm[j]) {  // new max: u' = a (u + s (m - mv)), s' = a s, a = e^(m - mv)
                    if (rs[j] > 0.0f) {
                        const float d = rm[j] - mv, al = __expf(d);
                        ru[j] = al * fmaf(rs[j], d, ru[j]);
                        rs[j] *= al;
                    }
                    rm[j] = mv;
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    if (n + r < V) {
                        const float d = x[r] - rm[j];
                        const float e = __expf(d);
                        rs[j] += e;
                        ru[j] = fmaf(e, d, ru[j]);
                    }
                }
                const unsigned off = (unsigned)(lab[j] - n);
                if (lab[j] >= 0 && off < 4u) {
                    xl[j] = off == 0 ? x[0] : off == 1 ? x[1] : off == 2 ? x[2] : x[3];
                    have[j] = true;
                }
            }
        }
    }

    // the 4 lanes of a row (fc = 0..3), then the two waves that share the rows (wn = 0, 1)
#pragma unroll
    for (int j = 0; j < FM; ++j) {
#pragma unroll
        for (int off = 16; off <= 32; off <<= 1) {
            const float mo = __shfl_xor(rm[j], off), so = __shfl_xor(rs[j], off), uo = __shfl_xor(ru[j], off);
            merge_state<float>(rm[j], rs[j], ru[j], mo, so, uo);
        }
    }
    if (wn == 1 && fc == 0) {
#pragma unroll
        for (int j = 0; j < FM; ++j) {
            s_red[wm][j * 16 + fr][0] = rm[j];
            s_red[wm][j * 16 + fr][1] = rs[j];
            s_red[wm][j * 16 + fr][2] = ru[j];
        }
    }
    __syncthreads();  // reached by every wave: no return above
#pragma unroll
    for (int j = 0; j < FM; ++j) {
        const int row = m0 + wm * 64 + j * 16 + fr;
        if (row >= M) continue;  // rows past M: nothing written
        if (wn == 0 && fc == 0) {
            merge_state<float>(rm[j], rs[j], ru[j], s_red[wm][j * 16 + fr][0], s_red[wm][j * 16 + fr][1],
                               s_red[wm][j * 16 + fr][2]);
            part[(int64_t)span * M + row] = f32x4{rm[j], rs[j], ru[j], 0.0f};
        }
        if (have[j]) xlab[row] = xl[j];
    }
}

// One thread per row: its spans merged in ascending order in float64, then nll = lse - x_label, ent = log S - U/S.
__global__ __launch_bounds__(256) void head_merge_kernel(const f32x4* __restrict__ part, const float* __restrict__ xlab,
                                                         int M, int V, int nspans, const int32_t* __restrict__ labels,
                                                         double* __restrict__ nll, double* __restrict__ ent) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= M) return;
    f32x4 p = part[r];
    double Mx = (double)p.x, S = (double)p.y, U = (double)p.z;
    for (int sp = 1; sp < nspans; ++sp) {
        p = part[(int64_t)sp * M + r];
        merge_state<double>(Mx, S, U, (double)p.x, (double)p.y, (double)p.z);
    }
    const double lse = Mx + log(S);
    if (ent) ent[r] = log(S) - U / S;
    if (nll) {
        const int lab = labels ? labels[r] : -1;
        nll[r] = (lab >= 0 && lab < V) ? lse - (double)xlab[r] : 0.0;
    }
}

static int spans_of(int V) {
    const int tiles = (V + BN - 1) / BN;
    return (tiles + HS_SPAN_TILES - 1) / HS_SPAN_TILES;
}

}  // namespace hs

}  // namespace nsg

extern "C" int ns_score_rows(const void* d_logits, int64_t ld, int64_t nrows, int V, int dtype,
                             const int32_t* d_labels, double* d_nll, double* d_entropy, void* hip_stream) {
    if (!d_logits || nrows < 0 || V <= 0 || ld < V) return NS_ERR_CONFIG;
    if (nrows == 0) return NS_OK;
    const size_t esz = dtype == NS_DTYPE_F16 ? 2 : 4;
    if (dtype != NS_DTYPE_F16 && dtype != NS_DTYPE_F32) return NS_ERR_CONFIG;
    if (((uintptr_t)d_logits & 15u) || ((ld * (int64_t)esz) & 15)) return NS_ERR_CONFIG;
    if (!d_nll && !d_entropy) return NS_OK;
    const int64_t blocks = (nrows + nsg::SC_WAVES - 1) / nsg::SC_WAVES;
    if (blocks > 0x7FFFFFFF) return NS_ERR_UNSUPPORTED;
    hipStream_t s = (hipStream_t)hip_stream;
    if (dtype == NS_DTYPE_F16)
        hipLaunchKernelGGL(nsg::score_rows_kernel<_Float16>, dim3((unsigned)blocks), dim3(64 * nsg::SC_WAVES), 0, s,
                           (const char*)d_logits, ld, nrows, V, d_labels, d_nll, d_entropy);
    else
        hipLaunchKernelGGL(nsg::score_rows_kernel<float>, dim3((unsigned)blocks), dim3(64 * nsg::SC_WAVES), 0, s,
                           (const char*)d_logits, ld, nrows, V, d_labels, d_nll, d_entropy);
    return hipGetLastError() == hipSuccess ? NS_OK : NS_ERR_HIP;
}

extern "C" int64_t ns_lm_head_score_work_bytes(int M, int V) {
    if (M <= 0 || V <= 0) return 0;
    return (int64_t)nsg::hs::spans_of(V) * M * 16 + (int64_t)M * 4;
}

extern "C" int ns_lm_head_score(const void* d_x, int64_t ldx, const void* d_wt, int64_t ldw, int M, int V, int K,
                                int logits_dtype, const int32_t* d_labels, double* d_nll, double* d_entropy,
                                void* d_work, int64_t work_bytes, void* hip_stream) {
    using namespace nsg::hs;
    if (!d_x || !d_wt || !d_work || M < 0 || V <= 0 || K <= 0) return NS_ERR_CONFIG;
    if (logits_dtype != NS_DTYPE_F16 && logits_dtype != NS_DTYPE_F32) return NS_ERR_CONFIG;
    if (ldx < K || ldw < K) return NS_ERR_CONFIG;
    const uintptr_t al = (uintptr_t)d_x | (uintptr_t)d_wt | (uintptr_t)d_work;
    if ((al & 15u) || (ldx & 7) || (ldw & 7) || ((uintptr_t)d_labels & 3u) ||
        (((uintptr_t)d_nll | (uintptr_t)d_entropy) & 7u))
        return NS_ERR_CONFIG;
    if (M == 0 || (!d_nll && !d_entropy)) return NS_OK;
    if (work_bytes < ns_lm_head_score_work_bytes(M, V)) return NS_ERR_CONFIG;
    if (K % BK || K > HS_MAX_K) return NS_ERR_UNSUPPORTED;  // more than one chain: the caller keeps the two launches
    const int nspans = spans_of(V);
    if (nspans > 65535) return NS_ERR_UNSUPPORTED;
    const dim3 grid((unsigned)((M + BM - 1) / BM), (unsigned)nspans);
    nsg::f32x4* part = (nsg::f32x4*)d_work;
    float* xlab = (float*)((char*)d_work + (int64_t)nspans * M * 16);
    hipStream_t s = (hipStream_t)hip_stream;
    if (logits_dtype == NS_DTYPE_F16)
        hipLaunchKernelGGL(head_score_kernel<true>, grid, dim3(NT), 0, s, (const f16*)d_x, ldx, (const f16*)d_wt, ldw, M,
                           V, K, d_labels, part, xlab);
    else
        hipLaunchKernelGGL(head_score_kernel<false>, grid, dim3(NT), 0, s, (const f16*)d_x, ldx, (const f16*)d_wt, ldw,
                           M, V, K, d_labels, part, xlab);
    hipLaunchKernelGGL(head_merge_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, s, part, xlab, M, V, nspans,
                       d_labels, d_nll, d_entropy);
    return hipGetLastError() == hipSuccess ? NS_OK : NS_ERR_HIP;
}
