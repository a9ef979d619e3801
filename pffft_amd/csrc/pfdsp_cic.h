// The CIC decimating down-converter of libpfdsp_cic_hip.so (reference: src/pf_cic.cpp, API include/pffft/pf_cic.h) and the
// carrier fill kernel (src/pf_carrier.cpp).  Included by pfdsp_cic_hip.hip; the host side and the ABI are there.
//
// The reference runs, per input sample, three int64 integrators (ig2 += ig1; ig1 += ig0; ig0 += x), restarts ig2 at every
// block of R samples and feeds it through two combs.  Everything is linear and int64 arithmetic wraps exactly, so the
// recurrence is regrouped without changing a bit:
//   * block moments S0 = sum x_i, A = sum u_i x_i, Q = sum u_i (u_i - 1)/2 x_i with u_i = R-1-i, summed here by lanes that
//     take every nseg-th sample of the block (coalesced reads) and run the integrator recurrence over their own samples;
//   * output k >= 2 is a closed form of the moments of blocks k-2, k-1, k (cic_out1 below): no scan over the call;
//   * outputs 0 and 1, the two outputs after every workgroup boundary and the outgoing state need the incoming state or a
//     neighbour's moments: the main kernel stores per-workgroup partials, cic_finish_kernel (same stream) does the rest.
// Two launches and no inter-workgroup hand-off inside a launch: stream-ordered and graph-capturable.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace pfcic {

typedef unsigned long long u64;
typedef long long i64;

constexpr int CIC_THREADS = 256;
constexpr int CIC_TCH = 16;                       // samples per lane per staged chunk of a block
constexpr int CIC_STAGE = CIC_THREADS * CIC_TCH;  // staged samples per pass (every block of the pass, one chunk)
constexpr int CIC_MAXCH = 64;                     // channels per launch (kernel argument block)
constexpr int CIC_MAXWG = 1024;                   // workgroups per launch = partial records per state
constexpr int CIC_TABLE = 4096;                   // packed (sin, cos) table: entry p = table[p] | table[p + 1024] << 16

enum { FMT_S16 = 0, FMT_CS16 = 1, FMT_CU8 = 2 };

// the two integrators, the two combs (component a, b) and the phase: what a call reads and advances
struct CicState {
    i64 ig0[2], ig1[2], comb0[2], comb1[2];
    u64 phase;
    u64 pad;
};
struct Moments {   // one block: S0, A, Q of components a and b
    i64 s[2], a[2], q[2];
};
struct CicPartial {  // one workgroup's share of one call
    i64 sum_s[2];      // sum of S0 over its blocks
    i64 sum_w[2];      // sum of R (K-1-k) S0(k) + A(k)
    Moments first[2];  // its first two blocks
    Moments last[2];   // its last two blocks
};
// device block of one state: CicState, the partial records, the table
constexpr size_t CIC_PARTIAL_OFF = 128;
constexpr size_t CIC_TABLE_OFF = CIC_PARTIAL_OFF + sizeof(CicPartial) * CIC_MAXWG;
constexpr size_t CIC_DEV_BYTES = CIC_TABLE_OFF + sizeof(uint32_t) * CIC_TABLE;
static_assert(sizeof(CicState) <= CIC_PARTIAL_OFF, "state header");

struct CicChan {
    char* dev;       // device block of the channel's state
    u64 freq;        // phase increment per input sample
    float2* out;     // outsize outputs
};
struct CicArgs {
    const void* in;
    u64 K;           // outputs per channel
    int R;           // decimation factor
    int nseg;        // lanes per block (power of two, <= 64)
    int nwg;         // workgroups = partial records written
    int nch;
    float gain;
    CicChan ch[CIC_MAXCH];
};

__host__ __device__ inline u64 wg_first_block(u64 K, int nwg, int w) { return (K * (u64)w) / (u64)nwg; }

// out1(k) for k >= 2 from the moments of blocks k-2, k-1, k (RR = R*R, T = R(R-1)/2, all mod 2^64)
__device__ __forceinline__ u64 cic_out1(const Moments& m2, const Moments& m1, const Moments& m0, int c, u64 R, u64 RR, u64 T) {
    return RR * (u64)m2.s[c] + R * ((u64)m1.a[c] - (u64)m2.a[c]) + T * ((u64)m1.s[c] - (u64)m2.s[c]) + (u64)m0.q[c] -
           2 * (u64)m1.q[c] + (u64)m2.q[c];
}

template <int FMT> struct InT;
template <> struct InT<FMT_S16> { typedef int16_t T; };
template <> struct InT<FMT_CS16> { typedef uint32_t T; };   // one int16 I/Q pair
template <> struct InT<FMT_CU8> { typedef uint16_t T; };    // one uint8 I/Q pair

// mixed sample (int32, cannot overflow for these operand ranges); tab = sin | cos << 16
template <int FMT>
__device__ __forceinline__ void cic_mix(typename InT<FMT>::T v, uint32_t tab, int& xa, int& xb) {
    const int s = (int16_t)(tab & 0xffffu), c = (int16_t)(tab >> 16);
    if constexpr (FMT == FMT_S16) {
        xa = (int)v * c;
        xb = (int)v * s;
    } else {
        int ma, mb;
        if constexpr (FMT == FMT_CS16) {
            ma = (int16_t)(v & 0xffffu);
            mb = (int16_t)(v >> 16);
        } else {
            ma = ((int)(v & 0xffu) << 8) - 32614;
            mb = ((int)(v >> 8) << 8) - 32614;
        }
        xa = ma * c - mb * s;
        xb = ma * s + mb * c;
    }
}

// One workgroup: the contiguous blocks [wg_first_block(w), wg_first_block(w+1)) of every channel, in passes of 256/nseg
// blocks.  Lane s of a block's group sums samples s, s+nseg, s+2 nseg, ... of the block; the pass's samples are staged
// through LDS in chunks of 16 per lane (one chunk when R <= 16 nseg, which the host's choice of nseg makes true up to R = 1024).
template <int FMT>
__global__ void __launch_bounds__(CIC_THREADS) cic_main_kernel(CicArgs a) {
    typedef typename InT<FMT>::T T;
    __shared__ uint32_t s_tab[CIC_TABLE];
    __shared__ T s_in[CIC_STAGE];
    __shared__ Moments s_m[2 + CIC_THREADS];       // [0], [1]: the two blocks before the pass; [2 + j]: block j of the pass
    __shared__ Moments s_ring[CIC_MAXCH][2];       // per channel: the last two blocks of the previous pass
    __shared__ u64 s_acc[CIC_MAXCH][4];            // per channel: sum_s[2], sum_w[2]

    const int tid = threadIdx.x, w = blockIdx.x;
    const u64 R = (u64)a.R, K = a.K;
    const int nseg = a.nseg, bpp = CIC_THREADS / nseg;
    const int s = tid & (nseg - 1), bi = tid / nseg;
    const u64 b0 = wg_first_block(K, a.nwg, w), b1 = wg_first_block(K, a.nwg, w + 1);
    const u64 RR = R * R, T_ = R * (R - 1) / 2;
    const int n_s = (a.R - s + nseg - 1) / nseg;   // samples of this lane in every block (nseg <= R: >= 1)
    const int nchunk = (a.R + nseg * CIC_TCH - 1) / (nseg * CIC_TCH);

    const uint32_t* g_tab = reinterpret_cast<const uint32_t*>(a.ch[0].dev + CIC_TABLE_OFF);
    for (int i = tid; i < CIC_TABLE; i += CIC_THREADS) s_tab[i] = g_tab[i];
    for (int i = tid; i < a.nch * 4; i += CIC_THREADS) s_acc[i >> 2][i & 3] = 0;
    const T* in = reinterpret_cast<const T*>(a.in);

    for (u64 pb = b0; pb < b1; pb += bpp) {
        const int nb = (int)((b1 - pb) < (u64)bpp ? (b1 - pb) : (u64)bpp);
        for (int c = 0; c < a.nch; ++c) {
            const u64 freq = a.ch[c].freq;
            const u64 ph0 = reinterpret_cast<const CicState*>(a.ch[c].dev)->phase;
            i64 p0[2] = {0, 0}, p1[2] = {0, 0}, p2[2] = {0, 0};
            for (int ck = 0; ck < nchunk; ++ck) {
                const int t0 = ck * CIC_TCH;
                if (nchunk > 1 || c == 0) {   // one chunk: the pass is staged once for every channel
                    __syncthreads();
                    const int per_blk = nseg * CIC_TCH, lg = __ffs(per_blk) - 1, lim = a.R - t0 * nseg;
                    // loads in flight in groups of 8 before their LDS stores (a thread stages <= CIC_TCH samples)
                    const T* pin = in + pb * R + (u64)(t0 * nseg);
#pragma unroll 1
                    for (int u0 = 0; u0 < CIC_TCH; u0 += 8) {
                        T v[8];
#pragma unroll
                        for (int u = 0; u < 8; ++u) {
                            const int i = tid + (u0 + u) * CIC_THREADS, j = i >> lg, r = i & (per_blk - 1);
                            if (i < nb * per_blk && r < lim) v[u] = pin[(u64)j * R + (u64)r];
                        }
#pragma unroll
                        for (int u = 0; u < 8; ++u) {
                            const int i = tid + (u0 + u) * CIC_THREADS, r = i & (per_blk - 1);
                            if (i < nb * per_blk && r < lim) s_in[i] = v[u];
                        }
                    }
                    __syncthreads();
                }
                if (bi < nb) {
                    const int tn = (n_s - t0) < CIC_TCH ? (n_s - t0) : CIC_TCH;
                    const u64 j0 = (pb + bi) * R + (u64)(t0 * nseg + s);
                    u64 ph = ph0 + j0 * freq;
                    const u64 step = (u64)nseg * freq;
                    const T* src = s_in + bi * (nseg * CIC_TCH) + s;
                    for (int t = 0; t < tn; ++t) {
                        int xa, xb;
                        cic_mix<FMT>(src[t * nseg], s_tab[ph >> 52], xa, xb);
                        ph += step;
                        p2[0] += p1[0]; p1[0] += p0[0]; p0[0] += xa;
                        p2[1] += p1[1]; p1[1] += p0[1]; p0[1] += xb;
                    }
                }
            }
            // the lane's samples are u = r_last + nseg * v (v = its reverse position): moments from its integrators
            Moments m;
            {
                const u64 beta = (u64)nseg;
                const u64 rl = (u64)(a.R - 1 - (s + (n_s - 1) * nseg));
                const u64 cq0 = rl * (rl - 1) / 2, cq1 = beta * rl + beta * (beta - 1) / 2, cq2 = beta * beta;
#pragma unroll
                for (int q = 0; q < 2; ++q) {
                    m.s[q] = p0[q];
                    m.a[q] = (i64)(rl * (u64)p0[q] + beta * (u64)p1[q]);
                    m.q[q] = (i64)(cq0 * (u64)p0[q] + cq1 * (u64)p1[q] + cq2 * (u64)p2[q]);
                }
            }
            for (int off = nseg >> 1; off > 0; off >>= 1) {
#pragma unroll
                for (int q = 0; q < 2; ++q) {
                    m.s[q] += __shfl_xor(m.s[q], off);
                    m.a[q] += __shfl_xor(m.a[q], off);
                    m.q[q] += __shfl_xor(m.q[q], off);
                }
            }
            __syncthreads();   // s_m of the previous channel is consumed
            if (s == 0 && bi < nb) s_m[2 + bi] = m;
            if (tid < 2) s_m[tid] = s_ring[c][tid];
            __syncthreads();
            u64 cs[2] = {0, 0}, cw[2] = {0, 0};
            if (tid < nb) {
                const u64 k = pb + tid;
                const Moments& m0 = s_m[2 + tid];
                if (k >= b0 + 2) {
                    const Moments &m1 = s_m[1 + tid], &m2 = s_m[tid];
                    a.ch[c].out[k] = make_float2((float)(i64)cic_out1(m2, m1, m0, 0, R, RR, T_) * a.gain,
                                                 (float)(i64)cic_out1(m2, m1, m0, 1, R, RR, T_) * a.gain);
                } else {
                    reinterpret_cast<CicPartial*>(a.ch[c].dev + CIC_PARTIAL_OFF)[w].first[k - b0] = m0;
                }
                const u64 rk = R * (K - 1 - k);
#pragma unroll
                for (int q = 0; q < 2; ++q) {
                    cs[q] = (u64)m0.s[q];
                    cw[q] = rk * (u64)m0.s[q] + (u64)m0.a[q];
                }
            }
            for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
                for (int q = 0; q < 2; ++q) {
                    cs[q] += __shfl_xor(cs[q], off);
                    cw[q] += __shfl_xor(cw[q], off);
                }
            }
            if ((tid & 63) == 0 && tid < nb) {
                atomicAdd(&s_acc[c][0], cs[0]); atomicAdd(&s_acc[c][1], cs[1]);
                atomicAdd(&s_acc[c][2], cw[0]); atomicAdd(&s_acc[c][3], cw[1]);
            }
            if (tid < 2) s_ring[c][tid] = s_m[nb + tid];
        }
    }
    __syncthreads();
    for (int c = tid; c < a.nch; c += CIC_THREADS) {
        CicPartial* P = reinterpret_cast<CicPartial*>(a.ch[c].dev + CIC_PARTIAL_OFF) + w;
        P->sum_s[0] = (i64)s_acc[c][0]; P->sum_s[1] = (i64)s_acc[c][1];
        P->sum_w[0] = (i64)s_acc[c][2]; P->sum_w[1] = (i64)s_acc[c][3];
        P->last[0] = s_ring[c][0]; P->last[1] = s_ring[c][1];
    }
}

// ig2 of a block from the integrators at its start: R g1 + T g0 + Q
__device__ __forceinline__ u64 cic_ig2(u64 g0, u64 g1, const Moments& m, int c, u64 R, u64 T) {
    return R * g1 + T * g0 + (u64)m.q[c];
}

// One workgroup per channel: folds the partials into the new state and writes the outputs the main kernel left out
// (0 and 1 from the incoming state, and the first two of every later workgroup from its neighbour's last two blocks).
__global__ void __launch_bounds__(CIC_THREADS) cic_finish_kernel(CicArgs a) {
    __shared__ u64 s_red[4][CIC_THREADS];
    const int tid = threadIdx.x;
    const CicChan ch = a.ch[blockIdx.x];
    CicState* st = reinterpret_cast<CicState*>(ch.dev);
    const CicPartial* P = reinterpret_cast<const CicPartial*>(ch.dev + CIC_PARTIAL_OFF);
    const u64 R = (u64)a.R, K = a.K, RR = R * R, T_ = R * (R - 1) / 2;
    const float g = a.gain;

    u64 acc[4] = {0, 0, 0, 0};
    for (int w = tid; w < a.nwg; w += CIC_THREADS) {
        acc[0] += (u64)P[w].sum_s[0]; acc[1] += (u64)P[w].sum_s[1];
        acc[2] += (u64)P[w].sum_w[0]; acc[3] += (u64)P[w].sum_w[1];
    }
    for (int w = 1 + tid; w < a.nwg; w += CIC_THREADS) {   // every workgroup holds >= 2 blocks when nwg > 1
        const u64 b = wg_first_block(K, a.nwg, w);
        const Moments &l0 = P[w - 1].last[0], &l1 = P[w - 1].last[1], &f0 = P[w].first[0], &f1 = P[w].first[1];
        ch.out[b] = make_float2((float)(i64)cic_out1(l0, l1, f0, 0, R, RR, T_) * g, (float)(i64)cic_out1(l0, l1, f0, 1, R, RR, T_) * g);
        ch.out[b + 1] = make_float2((float)(i64)cic_out1(l1, f0, f1, 0, R, RR, T_) * g, (float)(i64)cic_out1(l1, f0, f1, 1, R, RR, T_) * g);
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) s_red[q][tid] = acc[q];
    __syncthreads();
    if (tid != 0) return;
    for (int i = 1; i < CIC_THREADS; ++i)
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[q] += s_red[q][i];

    const CicState in = *st;
    CicState o = in;
    float2 out01[2];
    const Moments &M0 = P[0].first[0], &M1 = P[0].first[1];
    const Moments &Ml = P[a.nwg - 1].last[1], &Mp = P[a.nwg - 1].last[0];   // blocks K-1, K-2
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const u64 g0 = (u64)in.ig0[c], g1 = (u64)in.ig1[c];
        // outputs 0 and 1
        const u64 i2_0 = cic_ig2(g0, g1, M0, c, R, T_);
        const u64 o0_0 = i2_0 - (u64)in.comb0[c];
        const u64 o1_0 = o0_0 - (u64)in.comb1[c];
        (c == 0 ? out01[0].x : out01[0].y) = (float)(i64)o1_0 * g;
        if (K >= 2) {
            const u64 i2_1 = cic_ig2(g0 + (u64)M0.s[c], g1 + R * g0 + (u64)M0.a[c], M1, c, R, T_);
            const u64 o0_1 = i2_1 - i2_0;
            (c == 0 ? out01[1].x : out01[1].y) = (float)(i64)(o0_1 - o0_0) * g;
        }
        // new state
        const u64 n0 = g0 + acc[c], n1 = g1 + K * R * g0 + acc[2 + c];
        o.ig0[c] = (i64)n0;
        o.ig1[c] = (i64)n1;
        const u64 h0 = n0 - (u64)Ml.s[c], h1 = n1 - R * h0 - (u64)Ml.a[c];   // integrators at the start of block K-1
        const u64 i2_l = cic_ig2(h0, h1, Ml, c, R, T_);
        u64 i2_p;
        if (K >= 2) {
            const u64 e0 = h0 - (u64)Mp.s[c], e1 = h1 - R * e0 - (u64)Mp.a[c];
            i2_p = cic_ig2(e0, e1, Mp, c, R, T_);
        } else {
            i2_p = (u64)in.comb0[c];
        }
        o.comb0[c] = (i64)i2_l;
        o.comb1[c] = (i64)(i2_l - i2_p);
    }
    o.phase = in.phase + K * R * ch.freq;
    ch.out[0] = out01[0];
    if (K >= 2) ch.out[1] = out01[1];
    *st = o;
}

// carrier patterns: `period` scalars (8: four complex samples) repeated over n scalars
template <typename S>
__global__ void __launch_bounds__(CIC_THREADS) carrier_fill_kernel(S* out, u64 n, S p0, S p1, S p2, S p3, S p4, S p5, S p6,
                                                                   S p7) {
    const S pat[8] = {p0, p1, p2, p3, p4, p5, p6, p7};
    for (u64 i = (u64)blockIdx.x * CIC_THREADS + threadIdx.x; i < n; i += (u64)gridDim.x * CIC_THREADS) out[i] = pat[i & 7];
}

}  // namespace pfcic
